"""Scenes of the normal-integration pins (tests/test_normal_integration_ref_host.py, tests/test_gpu_normal_integration_pin.py): small
images whose masks are chosen for the places where the dense-box layout of csrc/sp_normals.hip can go wrong.  numpy only."""
import functools

import numpy as np

import normal_integration_ref as ref

STOP_SEED = 4         # stop_scene: chosen so that the float32 host CG's residuals fall strictly over k = 1..12 with no neighbouring
#                        pair within 1e-3 relative (held by test_normal_integration_ref_host.py)


def _normals(H, W, seed, patch=None):
    """curved_scene's normals at (H, W), 30 % sign-flipped (changes neither L nor b), with a patch of random unit normals."""
    rng = np.random.default_rng(seed)
    n = ref.curved_scene(H, W)[0].copy()
    flip = rng.uniform(size=(H, W)) < 0.3
    n[flip] = -n[flip]
    if patch is not None:
        r0, r1, c0, c1 = patch
        rnd = rng.standard_normal((r1 - r0, c1 - c0, 3))
        n[r0:r1, c0:c1] = rnd / np.linalg.norm(rnd, axis=-1, keepdims=True)
    return n.astype(np.float32)


def _camera(H, W):
    """fx != fy, the principal point off the pixel grid."""
    return np.array([[0.83 * W, 0, W / 2.0 - 0.7], [0, 0.74 * W, H / 2.0 + 0.3], [0, 0, 1]], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def setup_scene():
    """(normals (40,72,3) f32, K f32, names, masks (N,40,72) bool): one segment per mask --
    full rectangles bw in {15, 16, 17, 32, 33, 64} x bh in {1, 2, 5} (bw = 16, 32, 64: no padding column, element i + 1 of a row's last
    pixel is the next row's first), a single column, the whole image (flush with all four borders), and a ragged mask with holes,
    pixels joined only diagonally, isolated pixels and two components."""
    H, W = 40, 72
    names, masks = [], []
    for bw in (15, 16, 17, 32, 33, 64):
        for bh in (1, 2, 5):
            m = np.zeros((H, W), dtype=bool)
            r0, c0 = 3 + bh, 1 + (bw % 7)
            m[r0:r0 + bh, c0:c0 + bw] = True
            names.append(f"rect {bh}x{bw}")
            masks.append(m)
    m = np.zeros((H, W), dtype=bool)
    m[4:31, 11] = True
    names.append("column")
    masks.append(m)
    names.append("whole image")
    masks.append(np.ones((H, W), dtype=bool))
    rng = np.random.default_rng(21)
    m = np.zeros((H, W), dtype=bool)
    m[5:30, 9:50] = rng.uniform(size=(25, 41)) < 0.7            # ragged, with holes
    m[12:16, 20:26] = False                                      # a larger hole
    m[5:30, 36:38] = False                                       # ... cut into two components
    m[5, 9] = m[29, 49] = m[5, 49] = m[29, 9] = True
    m[32, 12] = m[33, 13] = m[34, 14] = m[33, 15] = True         # joined only diagonally
    m[36, 30] = m[2, 60] = True                                  # isolated
    names.append("ragged")
    masks.append(m)
    return _normals(H, W, 7, patch=(8, 20, 30, 52)), _camera(H, W), tuple(names), np.stack(masks)


@functools.lru_cache(maxsize=None)
def plan_batch_many():
    """300 masks of 8 x 16 (more than k_ni_layout's 256 threads): rectangles from few distinct sizes so that many len tie, with empty
    masks and single pixels among them.  (masks, None)."""
    rng = np.random.default_rng(300)
    masks = np.zeros((300, 8, 16), dtype=bool)
    for n in range(300):
        kind = rng.integers(0, 10)
        if kind == 0:
            continue                                             # empty
        if kind == 1:
            masks[n, rng.integers(0, 8), rng.integers(0, 16)] = True
            continue
        bh, bw = (1, 3, 8)[rng.integers(0, 3)], (2, 9, 16)[rng.integers(0, 3)]
        r0, c0 = rng.integers(0, 8 - bh + 1), rng.integers(0, 16 - bw + 1)
        masks[n, r0:r0 + bh, c0:c0 + bw] = rng.uniform(size=(bh, bw)) < 0.8
        masks[n, r0, c0] = masks[n, r0 + bh - 1, c0 + bw - 1] = True
    return masks, None


@functools.lru_cache(maxsize=None)
def plan_batch_mixed():
    """Masks of setup_scene with hints: none (-> the image), tight, loose, clipped to negative / beyond H, W, and an empty hint for an
    empty mask.  (masks (N,40,72), boxes (N,4) int32)."""
    _, _, names, masks = setup_scene()
    H, W = masks.shape[1:]
    pick = [names.index(k) for k in ("rect 5x17", "rect 1x64", "column", "whole image", "ragged", "rect 2x16", "rect 5x33", "rect 2x32")]
    masks = np.concatenate([masks[pick], np.zeros((2, H, W), dtype=bool)])
    tight = ref.plan_ref(masks)
    boxes = np.zeros((len(masks), 4), dtype=np.int32)
    for n in range(len(masks)):
        r0, c0, bh, bw = (int(tight[f][n]) for f in ("r0", "c0", "bh", "bw"))
        boxes[n] = [(0, 0, H, W), (r0, c0, r0 + bh, c0 + bw), (r0 - 2, c0 - 3, r0 + bh + 4, c0 + bw + 1), (-5, -9, H + 7, W + 3)][n % 4]
    boxes[-2] = (0, 0, H, W)                                     # an empty mask under a full hint
    boxes[-1] = (7, 9, 7, 9)                                     # ... and under an empty hint
    return masks, boxes


TIER_BH = (200, 201, 302, 303, 606, 607)     # bw = S = 64, len = (bh + 2) 64: 12928 / 12992 (3 len against NI_LDS_FLOATS), 19456 / 19520
#                                              (2 len), 38912 / 38976 (len); the labels only choose the shapes
TRIP_BH = (64, 65)                           # bh S = 4096 (one full trip of 1024 threads x 4 cells) and one row into the next trip


@functools.lru_cache(maxsize=None)
def tier_scene():
    """(normals (608,64,3) f32, K f32, masks (8,608,64) bool): bw = 64 segments of 85 % density whose first and last row and column are
    set (the tight box is the intended one), heights TIER_BH + TRIP_BH."""
    H, W = 608, 64
    rng = np.random.default_rng(64)
    r, c = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    n = np.stack([0.35 * np.sin(0.11 * c + 0.023 * r), 0.3 * np.cos(0.017 * r - 0.07 * c), np.ones((H, W))], -1)
    n += 0.05 * rng.standard_normal((H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    K = np.array([[77.3, 0, 31.4], [0, 71.9, 303.7], [0, 0, 1]], dtype=np.float32)
    masks = np.zeros((len(TIER_BH) + len(TRIP_BH), H, W), dtype=bool)
    for k, bh in enumerate(TIER_BH + TRIP_BH):
        r0 = (H - bh) // 2 if bh < 607 else 1
        m = rng.uniform(size=(bh, W)) < 0.85
        m[0] = m[-1] = True
        m[:, 0] = m[:, -1] = True
        masks[k, r0:r0 + bh] = m
    return n.astype(np.float32), K, masks


@functools.lru_cache(maxsize=None)
def stop_scene(seed=STOP_SEED):
    """(normals (34,48,3) f32, K f32, mask (34,48) bool): one ragged 30 x 40 segment."""
    H, W = 34, 48
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), dtype=bool)
    m[2:32, 5:45] = rng.uniform(size=(30, 40)) < 0.85
    m[2, 5:45] = m[31, 5:45] = True
    m[2:32, 5] = m[2:32, 44] = True
    return _normals(H, W, seed), _camera(H, W), m
