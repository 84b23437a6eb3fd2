"""Inputs of the point-table tests, shared by test_point_table_ref_host.py (which proves on the CPU what the GPU file relies on: exact
pyramids, validity margins, the position error behind ``point_table_ref.C_POS``, comparisons that notice seven planted errors) and
test_gpu_point_table.py.  numpy only; every keyframe is built from a fixed seed and carries its OWN intrinsics, whose principal point is
not the image centre.

Sizes (H, W) -- each the smallest that takes a path of the set-up:
    33 x 16      one 16-byte piece per row; N H is no multiple of the count pass's 64-row block
    64 x 1024    the widest fast-path row: 64 pieces, 64 bit words
    24 x 1040    wider than the fast path: byte count loop, two trips of the word fill
    50 x 84      4-byte words
    97 x 131     bytes; odd at every level
    5 x 3, 2 x 2 levels down to Wl = 2 and Wl = 1 (the scalar tap path); 2 x 2 also blurs a 1 x 1 level
    300 x 64     H > 256: more than one fill workgroup per segment
    1104 x 16    (N = 2) H > 1024: no bit-word fill, the boxed count pass in two chunks, the row scan's loop branch
    65 x 33      keypoints exactly half way between two pixels (0.5 (dim - 1) is 32 and 16: k + 0.5 is exact)
    33 x 16 'pp_outside'  the principal point lies OUTSIDE the image, so the segments that sample it read taps beyond the border

Segments of an ordinary keyframe (N = 11), by index:
    0  empty                        4  empty                              8  ragged blob, d ~ exp(-15): between 1e-7 and 1e-6 (zinv branch)
    1  the whole frame              5  one row with one pixel + a full row 9  pixels on odd rows only: off every even lattice
    2  corners, columns 15, 16, W-1 6  ragged blobs, ordinary depth       10  empty
    3  checkerboard                 7  ragged blob, d ~ exp(-17): below the 1e-7 floor
"""
import functools
import zlib

import numpy as np

f32 = np.float32

SIZES = [(33, 16), (64, 1024), (24, 1040), (50, 84), (97, 131), (5, 3), (2, 2), (300, 64), (1104, 16), (65, 33)]
CASE_NAMES = [f"{h}x{w}" for h, w in SIZES] + ["pp_outside"]
N_LEVELS = 3
SEG_EMPTY, SEG_FULL, SEG_SINGLES, SEG_CHECKER, SEG_ROWS, SEG_BLOBS, SEG_BELOW_FLOOR, SEG_ZINV, SEG_ODD_ROWS = (0, 4, 10), 1, 2, 3, 5, 6, 7, 8, 9
TIE_SEGMENTS = {SEG_FULL: (6, 7), SEG_BLOBS: (31, 4), SEG_BELOW_FLOOR: (20, 11), SEG_ZINV: (1, 14)}      # (row k, col k) of the k + 0.5 ties on 65 x 33


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def image(rng, H, W):
    """(3,H,W) float32, multiples of 1/256 in [1/16, 1]: a smooth wave plus noise, so that neighbouring taps differ (a wrong tap shows)
    while every level of a 4-level pyramid stays exact in float32 (dyadic weights: at most 8 + 4 l bits at level l)."""
    y, x = np.mgrid[0:H, 0:W]
    out = np.empty((3, H, W))
    for c in range(3):
        fy, fx, ph = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0), rng.uniform(0, 2 * np.pi)
        out[c] = 0.5 + 0.25 * np.sin(2 * np.pi * (fx * x / max(W, 4) + fy * y / max(H, 4)) + ph) + rng.uniform(-0.2, 0.2, size=(H, W))
    return (np.clip(np.rint(out * 256), 16, 256) / 256).astype(f32)


def blob(rng, H, W, n_discs=3):
    """ragged union of discs with random holes; never touches column 0 when the frame is wider than 4 (its box then starts off a 16-pixel
    boundary)"""
    y, x = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), bool)
    for _ in range(n_discs):
        r = rng.uniform(0.12, 0.3) * min(max(H, 6), max(W, 6))
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        m |= ((y - cy) / r) ** 2 + ((x - cx) / (r * rng.uniform(0.7, 2.5))) ** 2 <= 1
    m &= rng.uniform(size=(H, W)) < 0.85
    if W > 4:
        m[:, 0] = False
    if not m.any():
        m[H // 2, W // 2] = True
    return m


def _kp_of_pixel(px, dim):
    return f32(2.0 * px / (dim - 1) - 1.0)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, H, W, N, masks (N,H,W) bool, logdepth (N,H,W) f32, keypoints (N,2) f32, kld (N,) f32, K (3,3) f32, K_trg, image,
    trg_image (3,H,W) f32).  ``kld`` needs the keypoint log-depths: it is filled in by ``with_seeds`` below (from the reference's kp_L)."""
    pp_outside = name == "pp_outside"
    H, W = (33, 16) if pp_outside else tuple(int(v) for v in name.split("x"))
    rng = _rng("point_table", name)
    y, x = np.mgrid[0:H, 0:W]
    N = 2 if H == 1104 else 11
    masks = np.zeros((N, H, W), bool)
    if N == 2:
        masks[0] = True
        masks[1] = blob(rng, H, W, 6)
        masks[1, 200:300] = False                                   # a run of empty rows
    else:
        masks[SEG_FULL] = True
        for r, c in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, min(15, W - 1)), (H // 2, min(16, W - 1)), (H // 3, W - 1)):
            masks[SEG_SINGLES, r, c] = True
        masks[SEG_CHECKER] = (y + x) % 2 == 0
        masks[SEG_ROWS, H // 4, (2 * W) // 3] = True
        masks[SEG_ROWS, H - 1] = True
        masks[SEG_BLOBS] = blob(rng, H, W, 4)
        masks[SEG_BELOW_FLOOR] = blob(rng, H, W, 2)
        masks[SEG_ZINV] = blob(rng, H, W, 2)
        masks[SEG_ODD_ROWS] = (y % 2 == 1) & (rng.uniform(size=(H, W)) < 0.4)
        masks[SEG_ODD_ROWS, 1, W - 1] = True
    # log-depths: per segment a level plus a wave of amplitude <= 0.3 over the pixels, dense (the table reads them under the masks only)
    L = np.empty((N, H, W))
    for n in range(N):
        fy, fx, ph = rng.uniform(0.3, 1.5), rng.uniform(0.3, 1.5), rng.uniform(0, 2 * np.pi)
        L[n] = rng.uniform(-0.5, 0.8) + 0.2 * np.sin(2 * np.pi * (fx * x / max(W, 8) + fy * y / max(H, 8)) + ph) + rng.uniform(-0.1, 0.1, size=(H, W))
    L = L.astype(f32)
    # keypoints: a pixel of the frame per segment; one that wraps (pixel -1), one far outside (clamped); on 65 x 33 exact ties
    kp = np.empty((N, 2), f32)
    for n in range(N):
        kp[n] = (_kp_of_pixel(rng.integers(0, H), H), _kp_of_pixel(rng.integers(0, W), W))
    if N > 2:
        kp[SEG_CHECKER] = (f32(-1.0 - 2.0 / (H - 1)), _kp_of_pixel(W // 2, W))                 # row pixel -1: wraps to the last row
        kp[SEG_ROWS] = (f32(-5.0), f32(4.0))                                                      # far outside: row clamps to 0, column to W - 1
        kp[SEG_SINGLES, 1] = f32(-1.0 - 2.0 / (W - 1))                                          # column pixel -1: wraps to the last column
    if name == "65x33":
        for n, (kr, kc) in TIE_SEGMENTS.items():
            kp[n] = (f32((kr + 0.5) / 32.0 - 1.0), f32((kc + 0.5) / 16.0 - 1.0))
    fx_, fy_ = rng.uniform(0.8, 1.4) * W, rng.uniform(0.8, 1.4) * W
    cx, cy = (0.37 * (W - 1) + 0.113, 0.61 * (H - 1) - 0.071)
    if pp_outside:
        cx, cy = (W - 1) + 0.4, 0.61 * (H - 1) - 0.071
    K = np.array([[fx_, 0, cx], [0, fy_, cy], [0, 0, 1]], f32)
    K_trg = np.array([[fx_ * 1.01, 0, cx + 0.5], [0, fy_ * 0.99, cy - 0.25], [0, 0, 1]], f32)
    return dict(name=name, H=H, W=W, N=N, masks=masks, logdepth=L, keypoints=kp, K=K, K_trg=K_trg, image=image(rng, H, W), trg_image=image(rng, H, W),
                seed_offsets=rng.uniform(-0.2, 0.2, size=N))


def seeds(c, kp_L):
    """(N,) float32 log-depth seeds ``kld`` of a case from its keypoint log-depths (the reference's ``kp_L``): ordinary segments within
    0.2 of kp_L; the two tiny-depth segments so that d = exp(L + kld - kp_L) lies within exp(+-0.3) of exp(-17) and exp(-15) on every one
    of their pixels (1e-7 = exp(-16.1), 1e-6 = exp(-13.8))."""
    kld = kp_L.astype(np.float64) + c["seed_offsets"]
    if c["N"] > 2:
        for n, target in ((SEG_BELOW_FLOOR, -17.0), (SEG_ZINV, -15.0)):
            centre = 0.5 * (float(c["logdepth"][n].max()) + float(c["logdepth"][n].min()))
            kld[n] = kp_L[n] + target - centre
    return kld.astype(f32)


def nan_case():
    """A 9 x 12 keyframe of three segments; the middle one has NaN log-depths on all its pixels."""
    rng = _rng("point_table_nan")
    H, W, N = 9, 12, 3
    masks = rng.uniform(size=(N, H, W)) < 0.5
    L = rng.uniform(-0.3, 0.3, size=(N, H, W)).astype(f32)
    L[1] = np.nan
    kp = np.stack([(_kp_of_pixel(4, H), _kp_of_pixel(5, W))] * N).astype(f32)
    K = np.array([[11.0, 0, 4.6], [0, 12.5, 3.9], [0, 0, 1]], f32)
    return dict(name="nan", H=H, W=W, N=N, masks=masks, logdepth=L, keypoints=kp, K=K, K_trg=K.copy(), image=image(rng, H, W), trg_image=image(rng, H, W),
                kld=np.array([0.1, 0.2, -0.1], f32))
