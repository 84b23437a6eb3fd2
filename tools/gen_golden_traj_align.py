#!/usr/bin/env python
"""Write tests/golden/g26_traj_align.npz: what the REAL reference's ``align``, ``transfer_scale`` and ``apply_scale``
(tool/pose_utils.py:16-133) return on the shared cases of tests/traj_align_ref.py.

Needs the reference tree (SP_REFERENCE, as oracle/gen_goldens.py) at generation time only; the file holds data only: per case the
float32 input poses, the fields of ``align``'s dictionary, and for both ``anchor_rotation`` settings the poses ``transfer_scale``
returns (cases of at most 65 poses), its ``rot_reanchor`` and ``apply_scale`` of the second estimated pose.

    SP_REFERENCE=/path/to/reference python tools/gen_golden_traj_align.py
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import traj_align_ref as ref  # noqa: E402

REF = os.environ.get("SP_REFERENCE")

ALIGN_KEYS = ('rot', 'trans_scaled', 'trans_scaled_error', 'trans', 'trans_error', 's', 'model_aligned_scaled', 'model_aligned')


def reference_pose_utils():
    sys.path.insert(0, REF)                                      # (its ``from tool.etc import to_np``)
    try:
        spec = importlib.util.spec_from_file_location("reference_pose_utils", os.path.join(REF, "tool", "pose_utils.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(REF)
    return mod


def main():
    if not REF:
        sys.exit("set SP_REFERENCE to the reference tree")
    pose_utils = reference_pose_utils()
    out = {"names": np.array([c[0] for c in ref.CASES])}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # numpy.matrix / numpy.linalg.linalg deprecations
        for name, kind, n, seed in ref.CASES:
            pred, gt = ref.make_case(kind, n, seed)
            out[f"{name}_pred"], out[f"{name}_gt"] = pred, gt
            a = pose_utils.align(pred[:, :3, 3].T.astype(np.float64), gt[:, :3, 3].T.astype(np.float64))
            for key in ALIGN_KEYS:
                out[f"{name}_align_{key}"] = np.asarray(a[key], dtype=np.float64)
            for anchor in (False, True):
                est, pa = pose_utils.transfer_scale(list(gt.astype(np.float64)), list(pred.astype(np.float64)), anchor_rotation=anchor)
                tag = f"{name}_anchor{int(anchor)}"
                if n <= 65:                                       # (16 doubles a pose: kept for the short cases only)
                    out[f"{tag}_poses"] = np.stack(est)
                out[f"{tag}_has_reanchor"] = np.array('rot_reanchor' in pa)
                if 'rot_reanchor' in pa:
                    out[f"{tag}_rot_reanchor"] = np.asarray(pa['rot_reanchor'], dtype=np.float64)
                out[f"{tag}_applied"] = np.asarray(pose_utils.apply_scale(pred[1].astype(np.float64), pa), dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", "g26_traj_align.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(ref.CASES), "cases")


if __name__ == "__main__":
    main()
