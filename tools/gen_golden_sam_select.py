#!/usr/bin/env python
"""Write tests/golden/g25_sam_select.npz: what the REAL reference's ``frontend/segment/mask_generation.py`` ``infer_masks`` returns on
the synthetic SAM of tests/sam_select_ref.py, for the configurations A, B and C at 96x128 (40 + 12 keypoints) and 37x53 (12 + 4).

Needs the reference tree (SP_REFERENCE, as oracle/gen_goldens.py) at generation time only.  The three third-party modules the
reference file imports and this machine does not have (``segment_anything.utils.amg``, ``torchvision.ops.boxes``) and its
``frontend.segment.sam_tools`` (which imports ``segment_anything``) are stood in for by the helpers of tests/sam_select_ref.py: the
golden pins the reference's control flow and quirks on top of them, not the helpers themselves (tests/test_sam_select_host.py checks
those against brute force).  The file holds data only: logits as int8 multiples of 1/8, IoU predictions, keypoints, the sampler's
draws and every result tensor (masks bit-packed).

    SP_REFERENCE=/path/to/reference python tools/gen_golden_sam_select.py
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sam_select_ref as ref  # noqa: E402

REF = os.environ.get("SP_REFERENCE")
SEED = 7
counts = {"thresholds": [], "nms": [], "cut": [], "keypoint": []}       # (in, out) of every filter call


class RecordingMaskData(ref.MaskData):
    def __setitem__(self, key, value):
        old = self._stats.get(key)
        if key == "masks" and old is not None and old.dtype == torch.bool and value.dtype == torch.bool and old.dim() == 3:
            counts["cut"].append((int(old.sum()), int(value.sum())))
        super().__setitem__(key, value)

    def filter(self, keep):
        masks = self._stats.get("masks")
        if torch.is_tensor(keep) and keep.dtype == torch.bool and masks is not None and masks.dtype == torch.bool and masks.dim() == 3:
            counts["keypoint"].append((int(keep.numel()), int(keep.sum())))
        super().filter(keep)


def recording_nms(boxes, scores, idxs, iou_threshold):
    keep = ref.batched_nms(boxes, scores, idxs, iou_threshold)
    counts["nms"].append((int(boxes.shape[0]), int(keep.shape[0])))
    return keep


def reference_module():
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    for name in ("segment_anything", "segment_anything.utils", "torchvision", "torchvision.ops"):
        module(name)
    module("segment_anything.utils.amg", calculate_stability_score=ref.calculate_stability_score, batched_mask_to_box=ref.batched_mask_to_box,
           MaskData=RecordingMaskData)
    module("torchvision.ops.boxes", batched_nms=recording_nms, box_area=ref.box_area)
    module("frontend.segment.sam_tools", infer_sam_masks_batch=lambda model, image, keypoints: model(image, keypoints))
    sys.path.insert(0, REF)
    import frontend.segment.mask_generation as mg
    assert os.path.realpath(mg.__file__).startswith(os.path.realpath(REF)), mg.__file__
    return mg


def main():
    if not REF:
        sys.exit("set SP_REFERENCE to the reference tree")
    mg = reference_module()
    select, sample = mg.smallest_good_mask_batch, mg.active_sample_pos
    draws, no_good = [], []

    def recording_select(masks, iou_pred, **kw):
        out = select(masks, iou_pred, **kw)
        counts["thresholds"].append((int(masks.shape[0]) * (1 if kw["select_smallest"] else 3), int(out["masks"].shape[0])))
        if kw["select_smallest"] and kw["iou_threshold"] > 0 and kw["stability_score_thresh"] > 0:
            good = (iou_pred > kw["iou_threshold"]) & (ref.calculate_stability_score(masks, 0.0, 1.0) >= kw["stability_score_thresh"])
            no_good.append(int((~good.any(dim=1))[out["keypoints_ids"]].sum()))
        return out

    def recording_sample(coverage, num_samples=100, fine_noise=True):
        draws.append(sample(coverage, num_samples=num_samples, fine_noise=fine_noise))
        return draws[-1]

    mg.smallest_good_mask_batch, mg.active_sample_pos = recording_select, recording_sample
    out = {}
    for i, ((H, W), n1, n2, coarse) in enumerate(ref.SHAPES):
        keypoints = ref.golden_keypoints(n1)
        out[f"s{i}_keypoints"] = keypoints.numpy()
        for name, cfg in ref.CONFIGS.items():
            torch.manual_seed(100 + i)
            sam = ref.SyntheticSam(H, W, SEED)
            del draws[:]
            res = mg.infer_masks(sam, np.zeros((H, W, 3), np.float32), cfg, keypoints=keypoints, num_pts=n1, num_pts_active=n2,
                                 edge_probs_shape=ref.edge_shape_of(name, coarse), device=torch.device("cpu"))
            (q1, iou1), (q2, iou2) = sam.calls
            for v in (-8, 0, 8):
                assert bool((q1 == v).any()), f"no logit of exactly {v / 8}"
            if f"s{i}_logits1" in out:
                assert np.array_equal(out[f"s{i}_logits1"], q1.numpy())       # round 1 is the same for A, B and C
            out[f"s{i}_logits1"], out[f"s{i}_iou1"] = q1.numpy(), iou1.numpy()
            c = f"s{i}{name}_"
            out[c + "logits2"], out[c + "iou2"] = q2.numpy(), iou2.numpy()
            for k in ref.SAMPLER_ARRAYS:
                out[c + "sampler_" + k] = draws[0][k].numpy()
            arrays = ref.result_arrays(res)
            for k in ("masks", "coarse_coverage", "final_coverage"):
                arrays[k] = np.packbits(arrays[k], axis=-1)
            for k, v in arrays.items():
                out[c + k] = v
            print(f"{H}x{W} {name}: {3 * (n1 + n2)} candidates, {res['masks']['masks'].shape[0]} masks kept, num_active {res['num_active']}")
            if name == "C":
                gap = float((res["edge_probs"] - cfg["edge_probs_threshold"]).abs().min())
                print(f"   min |edge_probs - threshold| = {gap:.2e}")
                assert gap > 1e-4, gap
    for stage, io in counts.items():
        assert any(0 < o < n for n, o in io), (stage, io)                     # every filter both keeps and drops somewhere
        print(stage, io)
    assert sum(no_good) > 0, "no surviving keypoint without a good mask"
    print("surviving keypoints without a good mask:", no_good)
    path = os.path.join(ROOT, "tests", "golden", "g25_sam_select.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 600 * 1024, size


if __name__ == "__main__":
    main()
