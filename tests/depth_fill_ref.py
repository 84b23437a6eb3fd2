"""Yardsticks of the depth fill and the depth metrics, in numpy, and the inputs the tests of both share.

``nearest_valid_index`` restates the two-pass rule of DESIGN.md §4 "Depth fill": for every pixel the valid pixel that minimises
``(d^2, column, row)``.  ``scipy_index`` is scipy's own answer (what the reference's ``fill_depth`` indexes with).  ``metrics``
restates ``void.py:7-65`` with float32 terms and float64 sums."""
import numpy as np

OFF_NONE = -32768
METRIC_NAMES = ("n", "rmse", "mae", "absrel", "inv_rmse", "inv_mae", "inv_absrel", "delta105", "delta110", "delta1", "delta2", "delta3")
SHAPES = ((1, 7), (7, 1), (5, 300), (33, 65), (61, 83))
PATTERNS = ("holes", "sparse", "blobs", "checker")


# ---- the rule -------------------------------------------------------------------------------------------------------
def column_offsets(invalid):
    """Pass 1: ``r' - r`` of the nearest valid row of the pixel's column, the smaller row on a tie; OFF_NONE in a column without one."""
    H, W = invalid.shape
    r = np.arange(H)[:, None]
    above = np.maximum.accumulate(np.where(invalid, -1, r), axis=0)
    below = np.minimum.accumulate(np.where(invalid, H, r)[::-1], axis=0)[::-1]
    up = np.where(above >= 0, above - r, OFF_NONE)
    down = below - r
    take_down = (below < H) & ((up == OFF_NONE) | (down < -up))
    return np.where(take_down, down, up)


def nearest_valid_index(invalid):
    """Pass 2: flat index ``r' W + c'`` for every pixel.  Columns are visited c, c-1, c+1, c-2, c+2, ...: a column to the left wins on
    ``d^2 <= best`` (it is smaller than every column seen before), one to the right on ``d^2 < best`` only.  An image without a valid
    pixel maps every pixel to itself."""
    invalid = np.asarray(invalid, dtype=bool)
    H, W = invalid.shape
    off = column_offsets(invalid)
    have = off != OFF_NONE
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if not have.any():
        return (rows * W + cols).astype(np.int32)
    o2 = off.astype(np.int64) ** 2
    far = np.iinfo(np.int64).max
    best = np.where(have, o2, far)
    src_r = rows + np.where(have, off, 0)
    src_c = cols.copy()
    k = 1
    while k < W and k * k <= best.max():
        d = k * k + o2[:, :-k]                          # pixel (r, c) against column c - k
        win = have[:, :-k] & (d <= best[:, k:])
        best[:, k:][win] = d[win]
        src_r[:, k:][win] = (rows[:, :-k] + off[:, :-k])[win]
        src_c[:, k:][win] = cols[:, :-k][win]
        d = k * k + o2[:, k:]                           # ... and against column c + k
        win = have[:, k:] & (d < best[:, :-k])
        best[:, :-k][win] = d[win]
        src_r[:, :-k][win] = (rows[:, k:] + off[:, k:])[win]
        src_c[:, :-k][win] = cols[:, k:][win]
        k += 1
    return (src_r * W + src_c).astype(np.int32)


def scipy_index(invalid):
    """Flat index of ``distance_transform_edt(invalid, return_indices=True)`` -- needs at least one valid pixel."""
    from scipy import ndimage
    invalid = np.asarray(invalid, dtype=bool)
    ind = ndimage.distance_transform_edt(invalid, return_distances=False, return_indices=True)
    return (ind[0].astype(np.int64) * invalid.shape[1] + ind[1]).astype(np.int32)


def scipy_fill(depth, invalid):
    return depth.ravel()[scipy_index(invalid)].reshape(depth.shape)


# ---- inputs ---------------------------------------------------------------------------------------------------------
def unique_depth(H, W, seed):
    """Every pixel another float32 value, so equal values mean equal source pixels."""
    rng = np.random.default_rng(seed)
    return ((1 + rng.permutation(H * W)).astype(np.float32) / np.float32(1024)).reshape(H, W)


def invalid_mask(pattern, H, W, seed):
    rng = np.random.default_rng(seed)
    if pattern == "holes":                               # 15 % random holes
        m = rng.uniform(size=(H, W)) < 0.15
    elif pattern == "sparse":                            # 0.5 % valid: long searches, columns without a valid pixel
        m = rng.uniform(size=(H, W)) >= 0.005
    elif pattern == "blobs":                             # invalid discs, and the border rows and columns invalid throughout
        r, c = np.mgrid[:H, :W]
        m = np.zeros((H, W), dtype=bool)
        for _ in range(max(2, H * W // 12000)):
            r0, c0, rad = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(1, max(2.0, min(H, W) / 5))
            m |= (r - r0) ** 2 + (c - c0) ** 2 <= rad ** 2
        m[[0, -1], :] = True
        m[:, [0, -1]] = True
    elif pattern == "checker":                           # ties everywhere
        r, c = np.mgrid[:H, :W]
        m = (r + c) % 2 == 1
    else:
        raise ValueError(pattern)
    if m.all():                                          # the rule needs one valid pixel to be scipy's
        m[rng.integers(H), rng.integers(W)] = False
    return m


def fill_cases():
    """(name, invalid) of every small case: each shape under each pattern, and 2 x 2 with a single valid pixel."""
    out = []
    for si, (H, W) in enumerate(SHAPES):
        for pi, pattern in enumerate(PATTERNS):
            out.append((f"{pattern}_{H}x{W}", invalid_mask(pattern, H, W, 100 * si + pi)))
    one = np.ones((2, 2), dtype=bool)
    one[1, 0] = False
    out.append(("one_valid_2x2", one))
    return out


def metric_scene(seed=7, B=3, H=33, W=65):
    """Estimate, target and mask of B images: targets are inf outside the mask, and the last image has an empty mask."""
    rng = np.random.default_rng(seed)
    truth = rng.uniform(0.3, 4.5, size=(B, H, W)).astype(np.float32)
    estimate = (truth * np.exp(rng.normal(0, 0.08, size=truth.shape))).astype(np.float32)
    valid = rng.uniform(size=(B, H, W)) < 0.7
    valid[-1] = False
    target = np.where(valid, truth, np.float32(np.inf)).astype(np.float32)
    return estimate, target, valid


# ---- void.py:7-65 ---------------------------------------------------------------------------------------------------
def metrics(estimate, target, valid):
    """The twelve values of one image (METRIC_NAMES) as float64: terms in float32 as numpy forms them, sums in float64."""
    e = np.asarray(estimate, dtype=np.float32)[valid]
    t = np.asarray(target, dtype=np.float32)[valid]
    n = e.size

    def mean(x):
        assert x.dtype == np.float32
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.float64(np.sum(x, dtype=np.float64)) / np.float64(n)

    mm = np.float32(1000.0)
    km = np.float32(0.001)
    d = np.abs(mm * e - mm * t)
    inv_t = np.float32(1.0) / (km * t)
    di = np.abs(np.float32(1.0) / (km * e) - inv_t)
    ratio = np.maximum(t / e, e / t)
    below = [mean((ratio < np.float32(x)).astype(np.float32)) for x in (1.05, 1.10, 1.25, 1.25 ** 2, 1.25 ** 3)]
    return np.array([n, np.sqrt(mean(d * d)), mean(d), mean(d / (mm * t)), np.sqrt(mean(di * di)), mean(di), mean(di / inv_t)] + below,
                    dtype=np.float64)
