"""The float64 yardstick of the helpers that turn a segment table into a depth image (``csrc/sp_aux.hip``: ``sp_depth_splat``,
``sp_depth_splat_mean``, ``sp_segment_reinit`` with its invisible-segment fill, ``sp_depth_accumulate`` / ``sp_depth_average_finish``,
``sp_depth_expand``), restated in plain numpy from the header comments of ``include/sp_hip.h`` and the reference lines they cite
(``core/ops.py:59-96``, ``odometery/depth_init.py:10-67``, ``depth_completion/segment_based_completion.py:21-27``,
``core/dense_optim.py:38-80,164-174``).  Everything above the line "inputs of the tests" takes arrays and returns arrays and imports
nothing of the package; below it are the seeded inputs that ``test_segment_depth_ref_host.py`` (no GPU: is the yardstick right, are
the inputs decisive?) and ``test_gpu_segment_depth.py`` (the kernels against the yardstick) share.

What a render can be held to.  A point lands on the pixel (trunc v, trunc u).  Which pixel that is, is decided by the last bits of a
float32 ``exp`` and a division whenever u or v sits next to an integer, so a float64 statement cannot name the pixel of such a point --
but it knows WHICH points these are.  Every point within DELTA of a pixel border (or of the 1e-6 depth threshold) is ambiguous, and
every pixel an ambiguous point could land on is TAINTED; on all other pixels the touched set, the winner and the value are demanded
outright.  DELTA is a condition, not a measurement: the host test restates the positions in float32 (every intermediate rounded) and
asserts the gap to float64 at DELTA / 16 at most, and caps the tainted share of every input."""
from types import SimpleNamespace

import numpy as np

DELTA = 1e-3          # px: a point this close to a pixel border may land on either side in float32
RTOL = 2e-6           # render, average and expand values against float64 (about 16 ulp of float32)
TAU = 2e-6            # re-init values (|log(est) - L| <= 4: one logf, one subtraction, one addition)
EPS = 1e-6            # the reference's depth threshold, every use of it


# ---- the table ----------------------------------------------------------------------------------------------------------------------------
def keypoint_pixels(keypoints, H, W):
    """(N,2) int: the pixel a normalised (row, col) keypoint names -- float32 0.5 (size - 1) (kp + 1), round half to even."""
    kp = np.asarray(keypoints, np.float32)
    r = np.rint(np.float32(0.5) * np.float32(H - 1) * (kp[:, 0] + np.float32(1))).astype(np.int64)
    c = np.rint(np.float32(0.5) * np.float32(W - 1) * (kp[:, 1] + np.float32(1))).astype(np.int64)
    r, c = np.where(r < 0, r + H, r), np.where(c < 0, c + W, c)
    return np.stack([np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)], 1)


def make_table(masks, logdepth, keypoints):
    """Points in table order: segment by segment, row-major within a segment."""
    masks = np.asarray(masks, bool)
    N, H, W = masks.shape
    seg, row, col = np.nonzero(masks)
    L = np.asarray(logdepth, np.float64)
    kp = keypoint_pixels(keypoints, H, W)
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=N))])
    return SimpleNamespace(N=N, H=H, W=W, P=len(seg), seg=seg, row=row, col=col, L=L[seg, row, col], kp_L=L[np.arange(N), kp[:, 0], kp[:, 1]],
                           seg_off=seg_off)


# ---- render -------------------------------------------------------------------------------------------------------------------------------
def positions(t, K, kld, pose, dtype=np.float64):
    """(qz, u, v) of every table point: d = exp(L + (kld_n - kp_L_n)), unproject, rigid transform, project.  ``dtype`` = float32 rounds
    every intermediate to float32 (the host test's second statement, to bound what float32 can do to a position)."""
    f = lambda a: np.asarray(a, np.float64).astype(dtype)
    K, T, kld = f(K), f(pose), f(kld)
    with np.errstate(all="ignore"):
        d = np.exp(f(t.L) + (kld - f(t.kp_L))[t.seg])
        x = (f(t.col) - K[0, 2]) * d / K[0, 0]
        y = (f(t.row) - K[1, 2]) * d / K[1, 1]
        qx = T[0, 0] * x + T[0, 1] * y + T[0, 2] * d + T[0, 3]
        qy = T[1, 0] * x + T[1, 1] * y + T[1, 2] * d + T[1, 3]
        qz = T[2, 0] * x + T[2, 1] * y + T[2, 2] * d + T[2, 3]
        u = qx * K[0, 0] / qz + K[0, 2]
        v = qy * K[1, 1] / qz + K[1, 2]
    return qz, u, v


def _trunc(a):
    """truncation toward zero as an int64 (callers pass finite values below 2^62)"""
    return np.trunc(a).astype(np.int64)


def splat(t, K, kld, pose, mean=False, delta=DELTA):
    """The depth render.  A point is kept if qz > 1e-6, u and v are finite and (trunc v, trunc u) -- toward ZERO, so u in (-1, 0) is
    column 0 -- lies inside the image.  mean=False: the highest point index wins; mean=True: sum(qz) / (c + 1).  Untouched pixels 0.

    Returns image (H,W) f64, taint (H,W) bool, count (H,W) points per pixel, winner (H,W) highest point index or -1, and per point:
    pix (flat pixel or -1), qz, u, v."""
    H, W = t.H, t.W
    qz, u, v = positions(t, K, kld, pose)
    finite = np.isfinite(u) & np.isfinite(v)
    big = finite & (np.abs(u) < 2.0 ** 62) & (np.abs(v) < 2.0 ** 62)
    uc, vc = np.where(big, u, -2.0), np.where(big, v, -2.0)              # (what is not 'big' is not in the image)
    c, r = _trunc(uc), _trunc(vc)
    keep = (qz > EPS) & big & (r >= 0) & (r < H) & (c >= 0) & (c < W)
    pix = np.where(keep, r * W + c, -1)
    kp = pix[keep]
    count = np.bincount(kp, minlength=H * W)
    winner = np.full(H * W, -1, np.int64)
    np.maximum.at(winner, kp, np.nonzero(keep)[0])
    if mean:
        image = np.bincount(kp, weights=qz[keep], minlength=H * W) / (count + 1.0)
    else:
        image = np.where(winner >= 0, qz[np.maximum(winner, 0)], 0.0)
    # ambiguous points, and every pixel one of them could land on
    with np.errstate(invalid="ignore"):
        amb = (np.abs(u - np.rint(u)) < delta) | (np.abs(v - np.rint(v)) < delta) | (np.abs(qz - EPS) < 1e-7) | (~finite & (qz > EPS))
    amb &= big & ~(qz <= EPS - 1e-7) & ~np.isnan(qz)
    taint = np.zeros(H * W, bool)
    ua, va = u[amb], v[amb]
    for cc in (_trunc(ua - delta), _trunc(ua + delta)):
        for rr in (_trunc(va - delta), _trunc(va + delta)):
            ok = (rr >= 0) & (rr < H) & (cc >= 0) & (cc < W)
            taint[rr[ok] * W + cc[ok]] = True
    return SimpleNamespace(image=image.reshape(H, W), taint=taint.reshape(H, W), count=count.reshape(H, W), winner=winner.reshape(H, W),
                           pix=pix, qz=qz, u=u, v=v, ambiguous=amb)


# ---- re-init ------------------------------------------------------------------------------------------------------------------------------
def lower_median(a):
    a = np.sort(np.asarray(a, np.float64))
    return a[(len(a) - 1) // 2]


def reinit(t, est, mode):
    """Per segment: over its pixels with ``not (est < 1e-6)`` (a NaN is valid, as in the reference; est is float32 and so is the
    threshold) the mean or lower median of log(est) - L, plus kp_L; invisible segments: the lower median of the visible ones' results;
    nothing visible: zeros, every flag false.  Returns (kld (N,) f64, visible (N,) bool, sorted values per segment)."""
    assert mode in ("mean", "median")
    est = np.asarray(est, np.float32)
    e = est[t.row, t.col]
    valid = ~(e < np.float32(EPS))
    out, visible, values = np.zeros(t.N), np.zeros(t.N, bool), []
    for n in range(t.N):
        s = slice(t.seg_off[n], t.seg_off[n + 1])
        with np.errstate(all="ignore"):
            vals = np.sort(np.log(e[s][valid[s]].astype(np.float64)) - t.L[s][valid[s]])
        values.append(vals)
        if len(vals):
            visible[n] = True
            out[n] = (vals.mean() if mode == "mean" else vals[(len(vals) - 1) // 2]) + t.kp_L[n]
    if visible.any() and not visible.all():
        out[~visible] = lower_median(out[visible])
    return out, visible, values


# ---- average, expand ----------------------------------------------------------------------------------------------------------------------
def point_depths(t, kld):
    with np.errstate(all="ignore"):
        return np.exp(t.L + (np.asarray(kld, np.float64) - t.kp_L)[t.seg])


def average(t, kld, visible=None):
    """Per pixel the mean over the covering visible segments with d > 1e-6; divisor count + 1e-6; invalid iff count == 0.
    Returns (depth (H,W) f64, invalid (H,W) bool, count (H,W))."""
    d = point_depths(t, kld)
    use = d > EPS
    if visible is not None:
        use &= np.asarray(visible, bool)[t.seg]
    pix = (t.row * t.W + t.col)[use]
    count = np.bincount(pix, minlength=t.H * t.W)
    total = np.bincount(pix, weights=d[use], minlength=t.H * t.W)
    return (total / (count + 1e-6)).reshape(t.H, t.W), (count == 0).reshape(t.H, t.W), count.reshape(t.H, t.W)


def expand(masks, logdepth, keypoints, kld, log_space):
    """Dense (N,H,W): (L + (kld_n - kp_L_n)) * mask, or exp of that."""
    masks = np.asarray(masks, bool)
    N, H, W = masks.shape
    L = np.asarray(logdepth, np.float64)
    kp = keypoint_pixels(keypoints, H, W)
    shift = np.asarray(kld, np.float64) - L[np.arange(N), kp[:, 0], kp[:, 1]]
    out = (L + shift[:, None, None]) * masks
    return out if log_space else np.exp(out)


# ===========================================================================================================================================
# inputs of the tests (seeded; the host test shows that they are decisive, the GPU test runs the kernels on them)
# ===========================================================================================================================================
FAMILIES = {"blobs45x67": ((45, 67, 5), dict(shape="blobs", blob_coverage=1.3)),
            "grid33x50": ((33, 50, 4), dict(shape="grid", overlap=2)),
            "blobs40x56": ((40, 56, 4), dict(shape="blobs", blob_coverage=1.1))}
_pairs = {}


def family(name):
    """One ``synth.make_pair`` scene, seed 11 (a numpy generator of scenes; none of the code under test)."""
    if name not in _pairs:
        from super_primitive_amd import synth
        args, kw = FAMILIES[name]
        _pairs[name] = synth.make_pair(*args, seed=11, **kw)
    return _pairs[name]


def _translated(pose, t):
    out = np.array(pose, np.float32)
    out[:3, 3] += np.asarray(t, np.float32)
    return out


def far_pose(pair, table):
    """pose_gt moved back along z, doubling the distance until the render piles more than 3 points on a touched pixel on average"""
    s = 2.0
    while True:
        pose = _translated(pair.pose_gt, (0, 0, s))
        r = splat(table, pair.K, pair.kld_gt, pose, mean=True)
        if r.count.sum() > 3 * (r.count > 0).sum():
            return pose
        s *= 2.0
        assert s < 1e4


_render = {}


def render_cases(name):
    """{tag: (logdepth, kld, pose)} of one family.  gt / init: the scene's two poses.  shift: the image moved left and up by about a
    third, so a band of points has u or v in (-1, 0).  behind: everything behind the camera.  far (for the mean form): points piled
    up.  nan: segment 1's log-depth is NaN on every third masked pixel except its keypoint."""
    if name in _render:
        return _render[name]
    p = family(name)
    t = make_table(p.keypoint_regions, p.logdepth_perseg, p.keypoints)
    z = float(np.median(p.depth))
    shift = _translated(p.pose_init, (-(p.W / 3.0 + 0.37) * z / p.K[0, 0], -(p.H / 3.0 + 0.41) * z / p.K[1, 1], 0))
    behind = _translated(p.pose_gt, (0, 0, -(2.0 * float(point_depths(t, p.kld_init).max()) + 1.0)))
    L_nan = p.logdepth_perseg.copy()
    kp = keypoint_pixels(p.keypoints, p.H, p.W)
    rr, cc = np.nonzero(p.keypoint_regions[1])
    sel = (np.arange(len(rr)) % 3 == 0) & ~((rr == kp[1, 0]) & (cc == kp[1, 1]))
    L_nan[1, rr[sel], cc[sel]] = np.nan
    L = p.logdepth_perseg
    _render[name] = {"gt": (L, p.kld_gt, p.pose_gt), "init": (L, p.kld_init, p.pose_init), "shift": (L, p.kld_init, shift),
                     "behind": (L, p.kld_init, behind), "far": (L, p.kld_gt, far_pose(p, t)), "nan": (L_nan, p.kld_init, p.pose_init)}
    return _render[name]


def average_cases(name):
    """{tag: (kld, visible)}: no mask, all true, a mixed mask; in each, segment 2 sits at log-depth -20 (d <= 1e-6: skipped)."""
    p = family(name)
    kld = p.kld_init.copy()
    kld[2] = -20.0
    mixed = np.arange(p.N) % 3 != 1
    return {"none": (kld, None), "all": (kld, np.ones(p.N, bool)), "mixed": (kld, mixed)}


def _open_the_median(v, gap=3e-4):
    """v with the order statistics either side of its lower median pushed ``gap`` further apart (150 tau: a median that is off by one
    rank is off by far more than the comparison tolerance)"""
    order, k, out = np.argsort(v), (len(v) - 1) // 2, v.copy()
    out[order[k:]] += gap
    out[order[k + 1:]] += gap
    return out


def reinit_keyframe(tie=False):
    """The hand-made 48x80 keyframe of the re-init tests: (masks, logdepth, keypoints, est, meta).

    est: 15 % invalid (zeros and 5e-7, half each), a handful of 2e-6 (valid), the rest in [0.5, 8].  The valid pixels of a segment
    carry v = log(est) - L = centre_n + uniform(-0.3, 0.3); its invalid ones L = 0, so an invalid pixel taken for valid moves every
    statistic by a lot.  Every keypoint sits on an INVALID pixel of its mask whose L is the segment's 'lift': the result is the
    statistic plus the lift, and the lifts put the ten results 0.8 apart in a chosen order.

      0  3000 valid (even)      strided loops, lower median of an even count        5  zeros only: invisible
      1  3001 valid (odd)       strided loops, odd count                            6  values of both signs
      2  257 valid              just past one workgroup                             7  a plateau of equal values across the median rank
      3  256 valid              exactly one workgroup                               8  50 valid, the five largest values on est = 2e-6
      4  1 valid                smallest visible segment                            9  5e-7 only: invisible

    ``tie``: segment 8 becomes a copy of segment 6 -- two equal results at ranks 2 and 3 of the eight visible ones, so the fill's lower
    median (rank (8 - 1) // 2 = 3) is the SECOND of the pair and is found only through the index tie-break."""
    H, W, N = 48, 80, 10
    rng = np.random.default_rng(20241 + int(tie))
    u = rng.uniform(size=H * W)
    est = rng.uniform(0.5, 8.0, H * W).astype(np.float32)
    est[u < 0.15] = np.float32(5e-7)
    est[u < 0.075] = 0.0
    valid_px, zero_px, tiny_px = np.nonzero(u >= 0.15)[0], np.nonzero(u < 0.075)[0], np.nonzero((u >= 0.075) & (u < 0.15))[0]
    assert len(valid_px) >= 3101 and len(zero_px) >= 40 and len(tiny_px) >= 40
    small_px = valid_px[3150:3155]                                           # est = 2e-6 here: valid, only segment 8 covers them
    est[small_px] = np.float32(2e-6)
    plateau_px = valid_px[2000:2150]
    est[plateau_px] = np.float32(2.0)
    own = {0: valid_px[:3000], 1: valid_px[100:3101], 2: valid_px[200:457], 3: valid_px[1000:1256], 4: valid_px[3149:3150],
           5: zero_px[:40], 6: valid_px[500:1100], 7: np.concatenate([valid_px[1700:2000], plateau_px, valid_px[2150:2300]]),
           8: np.concatenate([valid_px[3100:3145], small_px]), 9: tiny_px[:40]}
    centre = {0: 1.0, 1: -1.0, 2: 1.0, 3: -1.0, 4: 1.0, 6: 0.0, 7: 0.0, 8: -1.0}
    # order of the results, lowest first; in the tie form 8 is 6 again, so the equal pair sits at ranks 2 and 3 of the visible eight
    order = [3, 0, 6, 8, 7, 2, 1, 4]
    lift = {n: 0.8 * (k - 3.5) - centre[n] for k, n in enumerate(order)}
    masks = np.zeros((N, H * W), bool)
    L = np.zeros((N, H * W), np.float32)
    kp_px = np.zeros(N, np.int64)
    loge = np.log(np.maximum(est.astype(np.float64), 1e-30))
    for n in range(N):
        px = own[n]
        masks[n, px] = True
        src = zero_px if n == 5 else tiny_px if n == 9 else (zero_px, tiny_px)[n % 2]
        extra = src[40 + 7 * n: 40 + 7 * n + 7]                                  # invalid pixels inside every mask
        masks[n, extra] = True
        kp_px[n] = extra[0]
        if n in centre:
            noise = _open_the_median(rng.uniform(-0.3, 0.3, len(px)))
            if n == 7:
                noise[300:450] = 0.011                                         # the plateau: est = 2, L the same everywhere on it
            if n == 8:
                noise = np.sort(noise)                                         # the five est = 2e-6 pixels carry the five largest values
            L[n, px] = (loge[px] - centre[n] - noise).astype(np.float32)
            L[n, kp_px[n]] = np.float32(lift[n])
    if tie:
        masks[8], L[8], kp_px[8] = masks[6], L[6], kp_px[6]
    keypoints = np.stack([2.0 * (kp_px // W) / (H - 1) - 1.0, 2.0 * (kp_px % W) / (W - 1) - 1.0], 1).astype(np.float32)
    meta = dict(plateau=7, invisible=[5, 9], tied=(6, 8) if tie else None)
    return masks.reshape(N, H, W), L.reshape(N, H, W), keypoints, est.reshape(H, W), meta


def reinit_rows():
    """300 single-row segments on a 30x64 image (the strided loops of the invisible-segment fill): segment n covers six pixels of row
    n % 30; every seventh segment (and one more, to leave an even number visible) sees only zeros."""
    H, W, N = 30, 64, 300
    rng = np.random.default_rng(3001)
    est = rng.uniform(0.5, 8.0, (H, W)).astype(np.float32)
    masks = np.zeros((N, H, W), bool)
    L = np.zeros((N, H, W), np.float32)
    kp = np.zeros((N, 2), np.int64)
    invisible = np.arange(N) % 7 == 3
    if (N - invisible.sum()) % 2:
        invisible[0] = True
    for n in range(N):
        r, c0 = n % 30, 6 * (n // 30)
        masks[n, r, c0:c0 + 6] = True
        kp[n] = (r, c0)
        if invisible[n]:
            est[r, c0:c0 + 6] = 0.0
        L[n, r, c0:c0 + 6] = (np.log(est[r, c0:c0 + 6].astype(np.float64) + (est[r, c0:c0 + 6] == 0)) - rng.uniform(-2.0, 2.0) - rng.uniform(-0.3, 0.3, 6)).astype(np.float32)
    keypoints = np.stack([2.0 * kp[:, 0] / (H - 1) - 1.0, 2.0 * kp[:, 1] / (W - 1) - 1.0], 1).astype(np.float32)
    return masks, L, keypoints, est, dict(invisible=np.nonzero(invisible)[0])


def expand_large():
    """One 520x512 segment: 266240 pixels, more than the 1024 blocks x 256 threads the expansion's grid is capped at."""
    H, W = 520, 512
    rng = np.random.default_rng(520512)
    masks = rng.uniform(size=(1, H, W)) < 0.7
    masks[0, 300, 200] = True
    L = (rng.uniform(0.3, 1.9, (1, H, W)) * masks).astype(np.float32)
    keypoints = np.array([[2.0 * 300 / (H - 1) - 1.0, 2.0 * 200 / (W - 1) - 1.0]], np.float32)
    return masks, L, keypoints, np.array([1.25], np.float32)
