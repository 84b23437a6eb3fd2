"""SAM mask selection as plain torch: the yardstick of tests/test_sam_select_host.py and tests/test_gpu_sam_select.py.

Two layers.  (1) The third-party helpers the reference's ``frontend/segment/mask_generation.py`` imports and this tree does not have
(``segment_anything.utils.amg``: stability score, mask to box, ``MaskData``; ``torchvision.ops.boxes``: ``box_area``, ``batched_nms``
with one category), restated from what they compute (DESIGN.md §4 "SAM mask selection").  tools/gen_golden_sam_select.py hands
exactly these to the REAL reference module as stand-ins, so golden g25 pins the reference's control flow on top of them.
(2) A restatement of the module itself on top of (1), which runs on CPU or GPU tensors and which g25 pins in turn.

Also here: the seeded synthetic "SAM" (nested noisy blobs, logits quantised to multiples of 1/8 so that values of exactly -1, 0 and
+1 occur) and the three configurations the tests use."""
import numpy as np
import torch
import torch.nn.functional as F

# ---- (1) third-party helpers ------------------------------------------------------------------------------------------


def threshold_count(x, t):
    """#(x > t) over the last two dimensions, int32 (strict; NaN is false)."""
    return (x > t).flatten(-2).sum(-1, dtype=torch.int32)


def calculate_stability_score(masks, mask_threshold, threshold_offset):
    return threshold_count(masks, mask_threshold + threshold_offset) / threshold_count(masks, mask_threshold - threshold_offset)


def batched_mask_to_box(masks):
    """XYXY int64 box of every bool mask (...,H,W): [min col, min row, max col, max row]; zeros for an empty mask."""
    H, W = masks.shape[-2:]
    if masks.numel() == 0:
        return torch.zeros(*masks.shape[:-2], 4, dtype=torch.int64, device=masks.device)
    rows, cols = masks.any(dim=-1), masks.any(dim=-2)
    r, c = torch.arange(H, device=masks.device), torch.arange(W, device=masks.device)
    top, bottom = torch.where(rows, r, H).amin(-1), torch.where(rows, r, -1).amax(-1)
    left, right = torch.where(cols, c, W).amin(-1), torch.where(cols, c, -1).amax(-1)
    box = torch.stack([left, top, right, bottom], dim=-1)
    return box * rows.any(dim=-1, keepdim=True)


def box_area(boxes):
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def nms(boxes, scores, iou_threshold):
    """Greedy NMS in float32: visit in falling score (equal scores: the lower index first), suppress j when
    inter / (area_i + area_j - inter) > threshold.  The kept indices in visiting order."""
    b = boxes.detach().float().cpu().numpy()
    order = torch.sort(scores.detach().float().cpu(), descending=True, stable=True)[1].numpy()
    b = b[order]
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    thr = np.float32(iou_threshold)
    dead = np.zeros(len(b), dtype=bool)
    keep = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for a in range(len(b)):
            if dead[a]:
                continue
            keep.append(order[a])
            w = np.maximum(np.minimum(b[a, 2], b[a + 1:, 2]) - np.maximum(b[a, 0], b[a + 1:, 0]), np.float32(0))
            h = np.maximum(np.minimum(b[a, 3], b[a + 1:, 3]) - np.maximum(b[a, 1], b[a + 1:, 1]), np.float32(0))
            inter = w * h
            dead[a + 1:] |= inter / (area[a] + area[a + 1:] - inter) > thr
    return torch.tensor(np.array(keep, dtype=np.int64), dtype=torch.int64, device=boxes.device)


def batched_nms(boxes, scores, idxs, iou_threshold):
    assert not bool(idxs.any()), "one category only"
    return nms(boxes, scores, iou_threshold)


class MaskData:
    """A dict of tensors that are filtered and concatenated together."""

    def __init__(self, **fields):
        self._stats = dict(fields)

    def __getitem__(self, key):
        return self._stats[key]

    def __setitem__(self, key, value):
        self._stats[key] = value

    def __delitem__(self, key):
        del self._stats[key]

    def items(self):
        return self._stats.items()

    def filter(self, keep):
        for k, v in self._stats.items():
            if v is not None:
                self._stats[k] = v[torch.as_tensor(keep, device=v.device)]

    def cat(self, other):
        for k, v in other.items():
            if self._stats.get(k) is None:
                self._stats[k] = v.clone()
            else:
                self._stats[k] = torch.cat([self._stats[k], v], dim=0)


# ---- (2) the module, restated -----------------------------------------------------------------------------------------


def normalise_coordinates(x_pixel, dims):
    return 2 * x_pixel * (1.0 / (torch.as_tensor(dims, dtype=torch.float32, device=x_pixel.device) - 1)) - 1


def denormalise_coordinates(x_norm, dims):
    return (0.5 * (torch.as_tensor(dims, dtype=torch.float32, device=x_norm.device) - 1) * (x_norm + 1)).round().long()


def smallest_good_mask_batch(masks, iou_pred, iou_threshold=0.88, stability_score_thresh=0.95, select_smallest=True):
    n, dev = masks.shape[0], masks.device
    tests = []
    if iou_threshold > 0:
        tests.append(iou_pred > iou_threshold)
    if stability_score_thresh > 0:
        tests.append(calculate_stability_score(masks, 0.0, 1.0) >= stability_score_thresh)
    binary = masks > 0.0
    if select_smallest:
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        good = torch.ones(n, 3, dtype=torch.bool, device=dev)
        for ok in tests:
            alive &= ok.any(dim=1)
            good &= ok
        size = threshold_count(masks, 0.0)
        size[~good] = 1000000
        s0, s1, s2 = size.unbind(dim=1)
        first_min = torch.where((s0 <= s1) & (s0 <= s2), 0, torch.where(s1 <= s2, 1, 2))
        ids = alive.nonzero()[:, 0]
        which = first_min[ids]
        out = {"masks": binary[ids, which], "iou_preds": iou_pred[ids, which], "keypoints_ids": ids, "masks_ids": which}
    else:
        ok = torch.ones(n, 3, dtype=torch.bool, device=dev)
        for t in tests:
            ok &= t
        cand = ok.reshape(-1).nonzero()[:, 0]
        out = {"masks": binary.flatten(0, 1)[cand], "iou_preds": iou_pred.reshape(-1)[cand],
               "keypoints_ids": torch.div(cand, 3, rounding_mode="floor")}
    out["boxes"] = batched_mask_to_box(out["masks"])
    return out


def coarse_density(coverage_mask, cell=16):
    covered = coverage_mask.clone()
    covered[:, -2:, :] = 1
    density = 1.0 - F.avg_pool2d(covered.float()[:, None], cell, stride=cell)
    return density / (density.sum(dim=(2, 3), keepdim=True) + 1e-6)


def active_sample_pos(coverage_mask, num_samples=100, fine_noise=True):
    B, H, W = coverage_mask.shape
    density = coarse_density(coverage_mask)
    Hc, Wc = density.shape[2:]
    flat = torch.distributions.Categorical(probs=density.view(B, -1)).sample((num_samples,)).view(num_samples, B)
    coarse_indices = torch.stack([flat // Wc, flat % Wc], dim=2).permute(1, 0, 2).reshape(B, num_samples, 2)
    coords = normalise_coordinates(coarse_indices, (Hc, Wc))
    if fine_noise:
        jitter = torch.randint_like(coords, high=8, device=coverage_mask.device)
        coords = (coords + (normalise_coordinates(jitter, (H, W)) + 1)).clamp(-1, 1)
    return {"coarse_density": density, "coarse_indices": coarse_indices,
            "sample_indices": denormalise_coordinates(coords, (H, W)).reshape(B, num_samples, 2),
            "normalised_coords": coords.reshape(B, num_samples, 2)}


def masks_to_edges(masks):
    """Scharr / 32 with reflect padding, from shifted slices (every product and sum is exact on 0/1 inputs, on any device)."""
    p = F.pad(masks[:, None].float(), (1, 1, 1, 1), mode="reflect")[:, 0]
    a, b, c = p[:, :-2], p[:, 1:-1], p[:, 2:]                     # rows r-1, r, r+1
    gx = (3 * (a[..., 2:] - a[..., :-2]) + 10 * (b[..., 2:] - b[..., :-2]) + 3 * (c[..., 2:] - c[..., :-2])) / 32
    gy = (3 * (c[..., :-2] - a[..., :-2]) + 10 * (c[..., 1:-1] - a[..., 1:-1]) + 3 * (c[..., 2:] - a[..., 2:])) / 32
    return torch.sqrt(gx * gx + gy * gy).amax(dim=0)


def infer_edge_probs(masks, pool_edges=False):
    edges = masks_to_edges(masks)
    if pool_edges:
        edges = F.max_pool2d(edges[None], kernel_size=3, stride=1, padding=1)[0]
    return edges, (1 - 2 * edges).clip(0, 1)


def nearest_resize(masks, shape):
    return F.interpolate(masks.float()[:, None], size=tuple(shape), mode="nearest")[:, 0] > 0.5


def infer_masks(sam, image, cfg, keypoints, num_pts_active, edge_probs_shape=None, sampler=None):
    H, W = image.shape[:2]
    sampler = active_sample_pos if sampler is None else sampler

    def one_round(kp):
        raw = sam(image, kp)
        data = MaskData(**smallest_good_mask_batch(raw["masks"], raw["iou_pred"], cfg["iou_threshold"], cfg["stability_threshold"],
                                                   cfg["select_smallest"]))
        kept = kp[data["keypoints_ids"]]
        if cfg["nms"]:
            scores = 1 / box_area(data["boxes"]) if cfg["filter_by_box_size"] else data["iou_preds"]
            keep = batched_nms(data["boxes"].float(), scores, torch.zeros_like(data["boxes"][:, 0]), cfg["box_nms_thresh"])
            data.filter(keep)
            kept = kept[keep]
        return data, kept

    data, keypoints_final = one_round(keypoints)
    coverage = data["masks"].any(dim=0)
    sampled, num_added = None, 0
    if num_pts_active > 0:
        sampled = sampler(coverage[None], num_pts_active)
        more, kept = one_round(sampled["normalised_coords"][0])
        num_added = kept.shape[0]
        keypoints_final = torch.cat([keypoints_final, kept], dim=0)
        data.cat(more)
    if edge_probs_shape is None:
        edges, edge_probs = infer_edge_probs(data["masks"])
        edges_coarse, probs_coarse = edges, edge_probs
    else:
        edges_coarse, probs_coarse = infer_edge_probs(nearest_resize(data["masks"], edge_probs_shape))
        edges = F.interpolate(edges_coarse[None, None], size=(H, W), mode="bilinear", align_corners=True)[0, 0]
        edge_probs = F.interpolate(probs_coarse[None, None], size=(H, W), mode="bilinear", align_corners=True)[0, 0]
    if cfg["cut_masks_by_edges"]:
        data["masks"] = data["masks"] & (edge_probs > cfg["edge_probs_threshold"])[None]
    if cfg["filter_edge_points"]:
        rc = denormalise_coordinates(keypoints_final, (H, W))
        at_keypoint = data["masks"][torch.arange(rc.shape[0], device=rc.device), rc[:, 0], rc[:, 1]]
        data.filter(at_keypoint)
        keypoints_final = keypoints_final[at_keypoint]
    return {"masks": data._stats, "keypoints": keypoints_final, "num_active": num_added, "coarse_coverage": coverage,
            "final_coverage": data["masks"].any(dim=0), "sampled_masks": sampled, "edges": edges, "edge_probs": edge_probs,
            "edge_coarse": edges_coarse, "edge_probs_coarse": probs_coarse}


# ---- the synthetic network, the configurations, the golden's layout ---------------------------------------------------

CONFIG_A = dict(select_smallest=True, nms=True, box_nms_thresh=0.8, iou_threshold=0.0, stability_threshold=0.90, filter_edge_points=True,
                cut_masks_by_edges=False, edge_probs_threshold=0.1, filter_by_box_size=False)        # the reference's config/tum values
CONFIG_B = dict(select_smallest=True, nms=True, box_nms_thresh=0.7, iou_threshold=0.88, stability_threshold=0.95, filter_edge_points=True,
                cut_masks_by_edges=True, edge_probs_threshold=0.5, filter_by_box_size=True)
CONFIG_C = dict(CONFIG_B, select_smallest=False, filter_by_box_size=False)
CONFIGS = {"A": CONFIG_A, "B": CONFIG_B, "C": CONFIG_C}
# (H, W), keypoints of round 1 and 2, the coarse edge shape of A and C (B takes its edges at full size)
SHAPES = (((96, 128), 40, 12, (36, 50)), ((37, 53), 12, 4, (21, 29)))
RESULT_ARRAYS = ("keypoints", "coarse_coverage", "final_coverage", "edges", "edge_probs", "edge_coarse", "edge_probs_coarse")
SAMPLER_ARRAYS = ("coarse_density", "coarse_indices", "sample_indices", "normalised_coords")


def edge_shape_of(name, coarse):
    return None if name == "B" else coarse


def golden_keypoints(n, seed=11):
    return torch.rand(n, 2, generator=torch.Generator().manual_seed(seed)) * 2 - 1


class SyntheticSam:
    """``(image, keypoints) -> {'masks': (n,3,H,W) logits, 'iou_pred': (n,3)}``: three nested noisy blobs around every keypoint,
    logits in multiples of 1/8, IoU predictions in [0.82, 1).  Keypoint 1 of every call is planted: its mask 0 passes IoU 0.88 but is
    unstable, its masks 1 and 2 are stable but fail IoU -- at B's thresholds it survives without a good mask.  Drawn on the host from
    its own generator, so the same seed gives the same logits on every device; ``calls`` keeps them as int8.  ``radius_scale`` shrinks the
    blobs (prompts drawn at random would otherwise cover the whole image at C's thresholds and leave round 2 nothing to sample)."""

    def __init__(self, H, W, seed, radius_scale=1.0):
        self.H, self.W, self.gen, self.calls, self.radius_scale = H, W, torch.Generator().manual_seed(seed), [], radius_scale

    def __call__(self, image, keypoints):
        H, W, g = self.H, self.W, self.gen
        kp = keypoints.detach().cpu().float()
        n = kp.shape[0]
        scale = self.radius_scale * min(H, W) / 48.0
        rad = (torch.rand(n, 1, generator=g) * 6 + 5) * scale * torch.tensor([1.0, 1.7, 2.6])
        slope = torch.rand(n, 3, generator=g) * 20 + 1
        iou = 0.82 + 0.18 * torch.rand(n, 3, generator=g)
        if n > 1:
            rad[1] = torch.tensor([5.0, 10.0, 15.0]) * scale * 1.3
            slope[1] = torch.tensor([0.2, 24.0, 24.0])
            iou[1] = torch.tensor([0.97, 0.83, 0.84])
        r0, c0 = (kp[:, 0] + 1) * 0.5 * (H - 1), (kp[:, 1] + 1) * 0.5 * (W - 1)
        d = torch.sqrt((torch.arange(H)[None, :, None] - r0[:, None, None]) ** 2 + (torch.arange(W)[None, None, :] - c0[:, None, None]) ** 2)
        logits = slope[:, :, None, None] * (rad[:, :, None, None] - d[:, None]) + 0.4 * torch.randn(n, 3, H, W, generator=g)
        q = (logits * 8).round().clamp(-127, 127)
        self.calls.append((q.to(torch.int8), iou))
        return {"masks": (q / 8).to(keypoints.device), "iou_pred": iou.to(keypoints.device)}


class ReplaySam:
    """Plays recorded calls back: ``rounds`` = [(int8 logits (n,3,H,W), iou (n,3)), ...] in call order."""

    def __init__(self, rounds):
        self.rounds, self.at = rounds, 0

    def __call__(self, image, keypoints):
        q, iou = self.rounds[self.at]
        self.at += 1
        assert q.shape[0] == keypoints.shape[0], (q.shape, keypoints.shape)
        q, iou = torch.as_tensor(q), torch.as_tensor(iou)
        return {"masks": (q.to(keypoints.device).float() / 8), "iou_pred": iou.to(keypoints.device)}


def golden_case(g, shape_index, name, device="cpu"):
    """What g25 holds for one case: (ReplaySam, keypoints, the recorded sampler, the expected result as a dict of numpy arrays)."""
    (H, W), n1, n2, coarse = SHAPES[shape_index]
    s, c = f"s{shape_index}_", f"s{shape_index}{name}_"
    rounds = [(g[s + "logits1"], g[s + "iou1"]), (g[c + "logits2"], g[c + "iou2"])]
    sampled = {k: torch.as_tensor(g[c + "sampler_" + k]).to(device) for k in SAMPLER_ARRAYS}
    want = {k: g[c + k] for k in RESULT_ARRAYS + ("iou_preds", "keypoints_ids", "boxes", "num_active")}
    if CONFIGS[name]["select_smallest"]:
        want["masks_ids"] = g[c + "masks_ids"]
    for k in ("coarse_coverage", "final_coverage"):
        want[k] = np.unpackbits(want[k], axis=-1, count=W).astype(bool)
    want["masks"] = np.unpackbits(g[c + "masks"], axis=-1, count=W).astype(bool)
    return ReplaySam(rounds), torch.as_tensor(g[s + "keypoints"]).to(device), (lambda coverage, n: sampled), want


def result_arrays(res):
    """The result of an infer_masks as the flat dict of numpy arrays ``golden_case`` returns."""
    out = {k: res[k].detach().cpu().numpy() for k in RESULT_ARRAYS}
    out.update({k: v.detach().cpu().numpy() for k, v in res["masks"].items()})
    out["num_active"] = np.int64(res["num_active"])
    return out


def assert_same_result(got, want, through_upsample, context=""):
    """Everything exact; the float maps bitwise, except edges / edge_probs behind the bilinear upsample: atol 1e-6."""
    assert set(got) == set(want), (context, sorted(set(got) ^ set(want)))
    for k in sorted(want):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (context, k, g.shape, w.shape)
        if through_upsample and k in ("edges", "edge_probs"):
            np.testing.assert_allclose(g, w, rtol=0, atol=1e-6, err_msg=f"{context} {k}")
        else:
            assert g.dtype == w.dtype, (context, k, g.dtype, w.dtype)
            assert np.array_equal(g, w, equal_nan=True), f"{context} {k}: {(g != w).sum()} of {g.size} differ"
