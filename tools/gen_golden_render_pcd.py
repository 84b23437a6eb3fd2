#!/usr/bin/env python
"""Write tests/golden/g_render_pcd.npz: what the REAL reference's ``tool/viz.py`` ``render_pcd`` returns on the two mode-0 cases of
tests/map_render_ref.py (``golden0``: 5003 points into 37 x 53 with points behind the camera; ``collide``: 70 001 points into 24 x 32).

Needs the reference tree (SP_REFERENCE, as oracle/gen_goldens.py) at generation time only.  ``tool/viz.py`` imports open3d,
matplotlib, cv2 and PIL at module level and ``render_pcd`` uses none of them: empty stand-in modules go into ``sys.modules``.  The
reference's K is float64 and NumPy forms u and v in float64; the points are handed over as float64 copies of the float32 inputs so
that this holds under every NumPy promotion rule.  The file holds data only: the image of each case, the inputs of the small case and,
for the large one (1.7 MB of random floats), the SHA-256 of the inputs the seeded generator of tests/map_render_ref.py must reproduce.

    SP_REFERENCE=/path/to/reference python tools/gen_golden_render_pcd.py
"""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import map_render_ref as ref  # noqa: E402

REF = os.environ.get("SP_REFERENCE")


def reference_module():
    for name in ("open3d", "matplotlib", "matplotlib.pyplot", "matplotlib.colors", "cv2", "PIL"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["matplotlib"].use = lambda *a, **k: None
    sys.path.insert(0, REF)
    import tool.viz as viz
    assert os.path.realpath(viz.__file__).startswith(os.path.realpath(REF)), viz.__file__
    return viz


def main():
    if not REF:
        sys.exit("set SP_REFERENCE to the reference tree")
    viz = reference_module()
    out = {}
    for name, make in ref.GOLDEN_CASES.items():
        case = make()
        pts, cols, K = case['points'], case['colours'], case['K']
        image = viz.render_pcd(pts.astype(np.float64), cols.astype(np.float64), K.astype(np.float64), case['H'], case['W'])
        assert image.dtype == np.uint8 and image.shape == (case['H'], case['W'], 3)
        mine, _, index = ref.render(pts, cols, K, None, case['H'], case['W'], 0)
        behind = int((pts[index[index >= 0], 2] < 0).sum())
        print(f"{name}: {len(pts)} points, {int((index >= 0).sum())} of {index.size} pixels hit, {behind} winners behind the camera, "
              f"statement equals the reference: {np.array_equal(mine, image)}")
        out[name + "_image"] = image
        out[name + "_sha256"] = np.array(ref.digest(case))
        if pts.nbytes < 100 * 1024:
            out[name + "_points"], out[name + "_colours"], out[name + "_K"] = pts, cols, K
    path = os.path.join(ROOT, "tests", "golden", "g_render_pcd.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 300 * 1024, size


if __name__ == "__main__":
    main()
