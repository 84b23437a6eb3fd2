"""Inputs of the keyframe post-processing tests, shared by test_post_process_ref_host.py (which proves on the CPU what the GPU file relies
on: narrow ambiguous bands, empty ones for the full stage, the shapes' structure) and test_gpu_post_process.py.  numpy only; every case is
built from a fixed seed, |L| <= 2 everywhere."""
import zlib

import numpy as np

f32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------------------
# sp_depth_discontinuity
# ---------------------------------------------------------------------------------------------------------------------------------
DISC_SHAPES = [(2, 2), (2, 9), (9, 2), (3, 3), (5, 255), (5, 256), (5, 257), (37, 53)]      # 255 / 256 / 257: around the 256-thread block
DISC_FILTERS = (1, 3, 5, 7)
DISC_THRESHOLDS = (0.1, 0.03)
MASK_KINDS = ("full", "random90", "isolated", "island", "empty_slice", "borders")
MAX_AMBIGUOUS_SHARE = 0.005


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def smooth_stepped_logdepth(rng, N, H, W):
    """A low-frequency wave (slopes on both sides of the thresholds) plus two rectangles per slice raised by a step; |L| <= 2."""
    y, x = np.mgrid[0:H, 0:W]
    L = np.zeros((N, H, W))
    for n in range(N):
        fy, fx, ph = rng.uniform(0.3, 1.2), rng.uniform(0.3, 1.2), rng.uniform(0, 2 * np.pi)
        L[n] = rng.uniform(-0.8, 0.8) + 0.35 * np.sin(2 * np.pi * (fx * x / max(W, 8) + fy * y / max(H, 8)) + ph)
        for _ in range(2):
            r0, c0 = rng.integers(0, H), rng.integers(0, W)
            r1, c1 = rng.integers(r0, H) + 1, rng.integers(c0, W) + 1
            L[n, r0:r1, c0:c1] += rng.choice([-0.5, 0.3, 0.6])
    return np.clip(L, -2, 2).astype(f32)


def valid_mask(kind, rng, N, H, W):
    y, x = np.mgrid[0:H, 0:W]
    v = np.ones((N, H, W), bool)
    if kind == "random90":
        v = rng.uniform(size=(N, H, W)) < 0.9
    elif kind == "isolated":                       # single valid pixels, none with a valid neighbour (8-connected)
        v[:] = (y % 2 == 0) & (x % 2 == 0)
    elif kind == "island":                         # a valid pixel inside a ring of invalid ones, valid beyond
        r, c = H // 2, W // 2
        v[:, max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = False
        v[:, r, c] = True
    elif kind == "empty_slice":
        v = rng.uniform(size=(N, H, W)) < 0.9
        v[N // 2] = False
    elif kind == "borders":                        # one segment that touches all four borders: the frame's rim and a cross
        v[:] = (y == 0) | (y == H - 1) | (x == 0) | (x == W - 1) | (y == H // 2) | (x == W // 2)
    return v


def disc_cases(shape):
    """Every (N, filter_size, threshold) at one shape; the mask kinds rotate so that each meets every filter size."""
    H, W = shape
    out = []
    i = DISC_SHAPES.index(shape)
    for N in (1, 3):
        for fs in DISC_FILTERS:
            for thr in DISC_THRESHOLDS:
                kind = MASK_KINDS[i % len(MASK_KINDS)]
                i += 1
                rng = _rng("disc", H, W, N, fs, thr)
                out.append(dict(name=f"{H}x{W}x{N}_fs{fs}_thr{thr}_{kind}", L=smooth_stepped_logdepth(rng, N, H, W),
                                valid=valid_mask(kind, rng, N, H, W), fs=fs, thr=thr))
    return out


def all_masks_case():
    """Every mask kind at 37 x 53 x 3 with the stage's own parameters (filter 3, threshold 0.1)."""
    out = []
    for kind in MASK_KINDS:
        rng = _rng("kinds", kind)
        out.append(dict(name=f"37x53x3_{kind}", L=smooth_stepped_logdepth(rng, 3, 37, 53), valid=valid_mask(kind, rng, 3, 37, 53), fs=3, thr=0.1))
    return out


RAMP_SHAPE = (5, 9)


def ramp_cases():
    """depth = 1 + s x, filter 1, all valid: the Scharr magnitude is s on the interior columns 1 .. W - 2 (the reflect padding makes it 0
    on the two border columns).  Four cases put s and the threshold 1e-4 relative = 1e-5 apart: several bands (disc_bound <= 14 U 1.8 =
    1.5e-6; float32 log-depths move the magnitude by less than 1e-7).  Two 'tight' ones put them 3e-5 relative = 3e-6 apart, two bands: a
    filter scale that is off by 5e-5 crosses.  expect: the discontinuity flag of every interior pixel; min_bands: what the host test
    asserts about the distance."""
    H, W = RAMP_SHAPE
    x = np.arange(W, dtype=np.float64)
    out = []
    for s, thr, expect, min_bands in ((0.1 * (1 + 1e-4), 0.1, True, 5), (0.1 * (1 - 1e-4), 0.1, False, 5),
                                      (0.1, 0.1 * (1 - 1e-4), True, 5), (0.1, 0.1 * (1 + 1e-4), False, 5),
                                      (0.1 * (1 + 3e-5), 0.1, True, 1.5), (0.1 * (1 - 3e-5), 0.1, False, 1.5)):
        L = np.broadcast_to(np.log(1 + s * x), (1, H, W)).astype(f32)
        out.append(dict(name=f"ramp_s{s:.7f}_thr{thr:.7f}", L=L, valid=np.ones((1, H, W), bool), fs=1, thr=thr, expect=expect, slope=s,
                        min_bands=min_bands))
    return out


def nonfinite_cases():
    """A two-level step image (so every finite gradient is 0 or 0.5) with NaN at a valid interior pixel and at a valid corner, +inf at a
    third valid pixel and NaN at an invalid one (which must not matter), for filter sizes 1 and 3."""
    H, W = 9, 11
    L = np.zeros((2, H, W), f32)
    L[:, :, 6:] = f32(np.log(2.0))
    valid = np.ones((2, H, W), bool)
    valid[:, 7, 1:4] = False
    L[0, 4, 3] = np.nan
    L[0, 0, 0] = np.nan
    L[0, 7, 2] = np.nan                     # invalid pixel
    L[1, 2, 8] = np.inf
    L[1, H - 1, W - 1] = np.nan
    L[1, 5, 2] = np.nan
    return [dict(name=f"nonfinite_fs{fs}", L=L.copy(), valid=valid.copy(), fs=fs, thr=0.1) for fs in (1, 3)]


# ---------------------------------------------------------------------------------------------------------------------------------
# sp_label_components
# ---------------------------------------------------------------------------------------------------------------------------------
def spiral(H, W):
    """A one-pixel-wide path from (0, 0) inwards, clockwise, with one-pixel gaps between its turns: ONE component whose root is pixel 0."""
    m = np.zeros((H, W), bool)
    r = c = 0
    dr, dc = 0, 1
    m[0, 0] = True

    def free(rr, cc):            # the cell can extend the path: inside, unset, and touching the path only at (r, c)
        if not (0 <= rr < H and 0 <= cc < W) or m[rr, cc]:
            return False
        touching = sum(1 for a, b in ((rr - 1, cc), (rr + 1, cc), (rr, cc - 1), (rr, cc + 1)) if 0 <= a < H and 0 <= b < W and m[a, b])
        return touching == 1
    while True:
        if not free(r + dr, c + dc):
            dr, dc = dc, -dr      # turn right: (0, 1) -> (1, 0) -> (0, -1) -> (-1, 0)
            if not free(r + dr, c + dc):
                return m
        r, c = r + dr, c + dc
        m[r, c] = True


def comb(H, W):
    """Teeth in every other column that join only in the last row: every merge between teeth arrives at the very end."""
    m = np.zeros((H, W), bool)
    m[:, ::2] = True
    m[H - 1] = True
    return m


def serpentine(H, W):
    m = np.zeros((H, W), bool)
    m[::2] = True
    m[1::4, W - 1] = True
    m[3::4, 0] = True
    return m


def checkerboard(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return (y + x) % 2 == 0


def nested_u(H, W):
    """U shapes open at the top, one inside the other, one pixel apart: the two arms of each meet only at its bottom."""
    m = np.zeros((H, W), bool)
    for k in range(0, min(H, W // 2) - 1, 2):
        m[0:H - k, k] = True
        m[0:H - k, W - 1 - k] = True
        m[H - 1 - k, k:W - k] = True
    return m


def bars(H, W):
    """Column 0 and column W - 1: two components that are neighbours in memory at every row end."""
    m = np.zeros((H, W), bool)
    m[:, 0] = True
    m[:, W - 1] = True
    return m


def label_cases():
    """name -> (N, H, W) bool."""
    rng = _rng("label")
    c = {
        "spiral_65x67": spiral(65, 67)[None],
        "comb_33x41": comb(33, 41)[None],
        "serpentine_34x29": serpentine(34, 29)[None],
        "checkerboard_16x18": checkerboard(16, 18)[None],         # even width: (r, 0) and (r - 1, W - 1) are both set
        "nested_u_21x40": nested_u(21, 40)[None],
        "full_full_7x9": np.ones((2, 7, 9), bool),
        "bars_after_full_6x5": np.stack([np.ones((6, 5), bool), bars(6, 5)]),
        "empty_between_5x6": np.stack([comb(5, 6), np.zeros((5, 6), bool), serpentine(5, 6)]),
        "row_1x300": (rng.uniform(size=(2, 1, 300)) < 0.7),
        "column_300x1": (rng.uniform(size=(2, 300, 1)) < 0.7),
        "one_pixel_set": np.ones((1, 1, 1), bool),
        "one_pixel_unset": np.zeros((3, 1, 1), bool),
        "width_257": np.stack([comb(4, 257), serpentine(4, 257), rng.uniform(size=(4, 257)) < 0.6]),
        "noise_mixed_30x33": rng.uniform(size=(3, 30, 33)) < np.array([0.45, 0.6, 0.75])[:, None, None],
    }
    return c


def big_spiral():
    return spiral(257, 259)[None]


# ---------------------------------------------------------------------------------------------------------------------------------
# sp_collect_parts / sp_build_part_masks: masks strictly contain split; slice 2 has an empty split
# ---------------------------------------------------------------------------------------------------------------------------------
def parts_case():
    rng = _rng("parts")
    N, H, W = 4, 19, 23
    split = rng.uniform(size=(N, H, W)) < 0.5
    split[1] = comb(H, W)
    split[2] = False
    masks = split | (rng.uniform(size=(N, H, W)) < 0.3)
    masks[3] = split[3]                            # and one slice where they coincide
    split[0, :, 11] = True                         # split pixels outside the mask exist too (the kernels AND with the mask)
    masks[0, 5:9, 11] = False
    return masks, split


# ---------------------------------------------------------------------------------------------------------------------------------
# sp_mask_count / sp_kth_mask_pixel
# ---------------------------------------------------------------------------------------------------------------------------------
def kth_masks():
    """name -> (H, W) bool.  'gaps' has empty leading, middle and trailing rows; 'last' has its only pixel at (H - 1, W - 1)."""
    rng = _rng("kth")
    gaps = np.zeros((11, 13), bool)
    gaps[2] = rng.uniform(size=13) < 0.5
    gaps[3, 12] = True
    gaps[6:8] = rng.uniform(size=(2, 13)) < 0.4
    gaps[8, 0] = True
    gaps[2, 4] = gaps[6, 0] = True
    last = np.zeros((7, 5), bool)
    last[6, 4] = True
    wide = rng.uniform(size=(3, 300)) < 0.3
    wide[1] = False
    return {"gaps_11x13": gaps, "last_7x5": last, "row_1x40": rng.uniform(size=(1, 40)) < 0.5, "column_40x1": rng.uniform(size=(40, 1)) < 0.5,
            "one_1x1": np.ones((1, 1), bool), "wide_3x300": wide}


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole stage at 40 x 50 (H W = 2000, so keep_ratio 1e-3 is exactly two pixels)
# ---------------------------------------------------------------------------------------------------------------------------------
STAGE_HW = (40, 50)
STAGE_RATIOS = (1e-3, 0.05)
STEP = float(f32(0.7))


def stage_case():
    """Five segments (log-depth steps of 0.7: the Scharr magnitude at a step is at least 0.5 (e^0.7 - 1) = 0.5, on two columns):
      0  rows 2..17, cols 2..47, steps at cols 16 and 32: components of 192, 224 and 256 pixels and a 64-pixel label-0 part
      1  rows 20..29, cols 2..21, step DOWN at col 18 (the pool puts the discontinuity on cols 18..19): components of 160 and 20 pixels, 20-pixel label-0 part
      2  the single pixel (22, 30)
      3  row 34, cols 6..17, steps at cols 10 and 15: components of 2, 3 and 3 pixels, 4-pixel label-0 part
      4  a disc of radius 8 around (30, 38) on a gentle ramp: one component, no label-0 part
    At keep_ratio 1e-3 (more than 2 pixels): 0 -> label-0 part first, then three parts; 1 -> three parts; 2 -> dropped; 3 -> label-0
    part and the two 3-pixel parts (the 2-pixel part sits exactly at the ratio); 4 -> whole.  At 0.05 (more than 100 pixels): 0 -> its
    three components; 1 -> one kept part, so the whole mask and its keypoint stay; 2, 3 -> dropped; 4 -> whole."""
    H, W = STAGE_HW
    y, x = np.mgrid[0:H, 0:W]
    N = 5
    L = np.zeros((N, H, W), f32)
    masks = np.zeros((N, H, W), bool)
    masks[0, 2:18, 2:48] = True
    L[0] = f32(-0.2) + STEP * ((x >= 16).astype(f32) + (x >= 32).astype(f32))
    masks[1, 20:30, 2:22] = True
    L[1] = f32(0.4) - STEP * (x >= 18).astype(f32)
    masks[2, 22, 30] = True
    L[2] = f32(0.1)
    masks[3, 34, 6:18] = True
    L[3] = f32(-0.5) + STEP * ((x >= 10).astype(f32) + (x >= 15).astype(f32))
    masks[4] = (y - 30) ** 2 + (x - 38) ** 2 <= 64
    L[4] = (0.2 + 0.004 * x + 0.002 * y).astype(f32)
    kp_px = np.array([[9, 40], [25, 20], [22, 30], [34, 7], [27, 41]], np.float64)
    keypoints = (2 * kp_px / (np.array([H, W]) - 1.0) - 1).astype(f32)
    expected = {1e-3: dict(K=11, sizes=[64, 192, 224, 256, 20, 160, 20, 4, 3, 3, 197]),
                0.05: dict(K=5, sizes=[192, 224, 256, 200, 197])}
    return dict(L=L, masks=masks, keypoints=keypoints, expected=expected)


def noisy_split_case():
    """One 64 x 96 slice whose split mask is noise on one colour of a checkerboard (about 2000 single-pixel components, more than the
    1024 rows post_process_kf collects at first) plus four blocks of 40 to 60 pixels, and a second, quiet slice.  keep_ratio 30 / 6144
    keeps the blocks and the label-0 part."""
    rng = _rng("noisy")
    H, W = 64, 96
    y, x = np.mgrid[0:H, 0:W]
    split = np.zeros((2, H, W), bool)
    split[0] = ((y + x) % 2 == 0) & (rng.uniform(size=(H, W)) < 0.7)
    for r0, c0, h, w in ((4, 6, 5, 8), (20, 50, 6, 10), (40, 10, 8, 5), (50, 70, 7, 8)):
        split[0, r0 - 1:r0 + h + 1, c0 - 1:c0 + w + 1] = False
        split[0, r0:r0 + h, c0:c0 + w] = True
    split[1, 10:30, 10:40] = True
    split[1, 40:50, 50:90] = True
    masks = split.copy()
    masks[0, 30:34, :] = True                       # the label-0 part of slice 0
    masks[1, 30:40, 20:30] = True                   # joins nothing: it lies outside split
    L = rng.uniform(-1, 1, size=(2, H, W)).astype(f32)
    kp_px = np.array([[6, 8], [15, 15]], np.float64)
    keypoints = (2 * kp_px / (np.array([H, W]) - 1.0) - 1).astype(f32)
    return dict(L=L, masks=masks, split=split, keypoints=keypoints, keep_ratio=30.0 / (H * W))
