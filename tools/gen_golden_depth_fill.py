#!/usr/bin/env python
"""Write tests/golden/g24_depth_fill.npz: what the REAL reference's ``fill_depth`` (depth_completion/fill_in_tools.py:5-7) and
``ErrorMetricsDeltas`` (depth_completion/void.py:67-97) return on the shared inputs of tests/depth_fill_ref.py.

Needs the reference tree (SP_REFERENCE, as oracle/gen_goldens.py) at generation time only; the file holds data only: the names of
the fill cases, their packed invalid masks, depths and filled outputs, and the metric scene with the reference's twelve values
per image (n, then the attributes rmse .. inv_absrel, delta105, delta110, delta1, delta2, delta3).

    SP_REFERENCE=/path/to/reference python tools/gen_golden_depth_fill.py
"""
import importlib.util
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import depth_fill_ref as ref  # noqa: E402

REF = os.environ.get("SP_REFERENCE")


def reference_module(name):
    spec = importlib.util.spec_from_file_location("reference_" + name, os.path.join(REF, "depth_completion", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    if not REF:
        sys.exit("set SP_REFERENCE to the reference tree")
    fill_in_tools, void = reference_module("fill_in_tools"), reference_module("void")
    out = {}
    names = []
    for k, (name, invalid) in enumerate(ref.fill_cases()):
        H, W = invalid.shape
        depth = ref.unique_depth(H, W, 1000 + k)
        names.append(name)
        out[f"fill{k}_shape"] = np.array([H, W], dtype=np.int32)
        out[f"fill{k}_invalid"] = np.packbits(invalid, axis=-1)
        out[f"fill{k}_depth"] = depth
        out[f"fill{k}_filled"] = fill_in_tools.fill_depth(depth, invalid).astype(np.float32)
    out["fill_names"] = np.array(names)
    estimate, target, valid = ref.metric_scene()
    values = np.empty((len(valid), len(ref.METRIC_NAMES)), dtype=np.float64)
    for b in range(len(valid)):
        m = void.ErrorMetricsDeltas()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                       # the empty mask: numpy's "mean of empty slice"
            m.compute(estimate[b], target[b], valid[b])
        values[b] = [valid[b].sum()] + [getattr(m, name) for name in ref.METRIC_NAMES[1:]]
    out["metric_estimate"], out["metric_target"] = estimate, target
    out["metric_valid"] = np.packbits(valid, axis=-1)
    out["metric_values"] = values
    path = os.path.join(ROOT, "tests", "golden", "g24_depth_fill.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(names), "fill cases")


if __name__ == "__main__":
    main()
