"""NumPy float64 statements of the map consistency test and of the keyframes' own depth images (include/sp_hip.h: sp_map_consistency,
sp_keyframe_depths), independent of the kernels: the projection is tests/map_render_ref.py's, every window is decided by an explicit
loop over its pixels and every keyframe-depth winner by an explicit loop over the table points.  The inputs of every device case are
made here too, so that the host tests can check them.

Ambiguity mask (the role position_taint plays for the renderer).  Under a non-identity pose u, v and z are float64 sums whose last bit
depends on the order they are formed in, so a pair (point, view) is ambiguous if u or v lies within DELTA px of an integer (the pixel,
and with it the window, may move), or if for some valid window pixel the point sits on a class border: | |zf - D| - b | <= 1e-9 D, or
|z - z_min| <= 1e-9.  With the identity pose there is no sum at all and nothing is ambiguous.  A point is ambiguous if any of its
pairs is; it may then differ from the statement by one view per ambiguous pair moving between two classes."""
import numpy as np

import map_render_ref as render_ref
from map_render_ref import DELTA, Z_MIN, camera, pose_of, project

AGREE, IN_FRONT, BEHIND, UNSEEN, SKIPPED = 0, 1, 2, 3, 4
CLASS_NAMES = ("agree", "in_front", "behind", "unseen", "skipped")
BORDER_RTOL = 1e-9


def _cameras(Ks, V):
    Ks = np.asarray(Ks, np.float32)
    return np.broadcast_to(Ks, (V, 3, 3)) if Ks.ndim == 2 else Ks


def classify_window(zf, values, tol64):
    """One pair: ``values`` are the float32 depths of the window's pixels (any order).  Returns the class."""
    any_valid, agree, all_front = False, False, True
    for d32 in values:
        D = np.float64(d32)
        if not (D > 0.0 and D < np.inf):
            continue
        any_valid = True
        b = tol64 * D
        if abs(zf - D) <= b:
            agree = True
        if not zf < D - b:
            all_front = False
    if not any_valid:
        return UNSEEN
    return AGREE if agree else (IN_FRONT if all_front else BEHIND)


def window_pixels(r, c, window, H, W):
    return [(rr, cc) for rr in range(max(r - window, 0), min(r + window, H - 1) + 1) for cc in range(max(c - window, 0), min(c + window, W - 1) + 1)]


def classes(points, Ks, poses, depth, owner=None, view_owner=None, tol=0.05, window=1, z_min=Z_MIN):
    """(Q,V) int8: the class of every pair, by a loop over the seen pairs and an explicit loop over each window's pixels."""
    points = np.asarray(points, np.float32)
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    Ks = _cameras(Ks, V)
    Q = len(points)
    tol64, zmin64 = np.float64(np.float32(tol)), np.float64(np.float32(z_min))
    out = np.full((Q, V), UNSEEN, np.int8)
    for j in range(V):
        u, v, z = project(points, Ks[j], poses[j])
        with np.errstate(invalid='ignore', over='ignore'):
            seen = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (z > zmin64)
            zf = z.astype(np.float32).astype(np.float64)
        skip = np.zeros(Q, bool)
        if owner is not None and view_owner is not None:
            skip = (np.asarray(owner) == view_owner[j]) & (view_owner[j] >= 0)
        out[skip, j] = SKIPPED
        img = depth[j]
        for i in np.nonzero(seen & ~skip)[0]:
            r, c = int(v[i]), int(u[i])
            out[i, j] = classify_window(zf[i], [img[rr, cc] for rr, cc in window_pixels(r, c, window, H, W)], tol64)
    return out


def counts_of(cls):
    """(Q,3) int32 from the (Q,V) classes: the views of each of agree / in_front / behind."""
    return np.stack([(cls == k).sum(axis=1) for k in (AGREE, IN_FRONT, BEHIND)], axis=1).astype(np.int32)


def ambiguous(points, Ks, poses, depth, tol=0.05, window=1, z_min=Z_MIN, delta=DELTA):
    """(Q,V) bool: the pairs whose class may depend on the last bit of a float64 sum (see the module's docstring)."""
    points = np.asarray(points, np.float32)
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    Ks = _cameras(Ks, V)
    tol64, zmin64 = np.float64(np.float32(tol)), np.float64(np.float32(z_min))
    out = np.zeros((len(points), V), bool)
    for j in range(V):
        if render_ref.is_identity(poses[j]):
            continue
        u, v, z = project(points, Ks[j], poses[j])
        with np.errstate(invalid='ignore', over='ignore'):
            finite = np.isfinite(u) & np.isfinite(v)
            edge = finite & ((np.abs(u - np.round(u)) <= delta) | (np.abs(v - np.round(v)) <= delta))
            near = np.abs(z - zmin64) <= BORDER_RTOL
            seen = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (z > zmin64)
            zf = z.astype(np.float32).astype(np.float64)
        out[:, j] = edge | near
        img = depth[j].astype(np.float64)
        for i in np.nonzero(seen & ~out[:, j])[0]:
            for rr, cc in window_pixels(int(v[i]), int(u[i]), window, H, W):
                D = img[rr, cc]
                if D > 0.0 and D < np.inf and abs(abs(zf[i] - D) - tol64 * D) <= BORDER_RTOL * D:
                    out[i, j] = True
    return out


def check_counts(got, cls, amb, what=""):
    """``got`` (Q,3) against the statement: exact on every unambiguous point; an ambiguous point may differ by one view per ambiguous
    pair moving between two classes (unseen is one of them).  Returns the number of ambiguous points."""
    want = counts_of(cls)
    got = np.asarray(got)
    assert got.dtype == np.int32 and got.shape == want.shape, what
    n_amb = amb.sum(axis=1)
    clean = n_amb == 0
    np.testing.assert_array_equal(got[clean], want[clean], err_msg=what)
    moved = np.abs(got.astype(np.int64) - want).sum(axis=1)
    assert np.all(moved[~clean] <= 2 * n_amb[~clean]), what
    return int((~clean).sum())


# ---- the keyframes' own depth images ------------------------------------------------------------------------------------------------
def decode_pix(pix):
    """(row, col) of the table's packed pixels (csrc/sp_device.h decode_pix: col = bits 0..15, row = bits 16..30)."""
    w = np.asarray(pix).astype(np.int64) & 0xffffffff
    return ((w >> 16) & 0x7fff).astype(np.int64), (w & 0xffff).astype(np.int64)


def keyframe_depth(rows, cols, z, seg_of_point, H, W):
    """One keyframe: depth (H,W) float32 and seg (H,W) int32 by a loop over the table points in ascending index; a point takes the pixel
    when its z is smaller than or EQUAL to the holder's (it has the higher index); a z that is not a finite float > 0 is skipped."""
    depth = np.zeros((H, W), np.float32)
    seg = np.full((H, W), -1, np.int32)
    z = np.asarray(z, np.float32)
    for i in range(len(z)):
        if not (z[i] > 0 and z[i] < np.inf):
            continue
        r, c = rows[i], cols[i]
        if seg[r, c] < 0 or z[i] <= depth[r, c]:
            depth[r, c], seg[r, c] = z[i], seg_of_point[i]
    return depth, seg


# ---- the inputs of the device cases -------------------------------------------------------------------------------------------------
def _spoil(depth, rng, zeros=0.1):
    """10 % zeros plus a few NaN, negative and +inf pixels, in place."""
    kind = rng.uniform(size=depth.shape)
    depth[kind < zeros] = 0.0
    depth[(kind >= zeros) & (kind < zeros + 0.01)] = np.nan
    depth[(kind >= zeros + 0.01) & (kind < zeros + 0.02)] = -1.5
    depth[(kind >= zeros + 0.02) & (kind < zeros + 0.03)] = np.inf
    return depth


def case_posed():
    """Q = 5003 (20 workgroups, the last one partial) in the box of map_render_ref.case_posed, its three posed views of 30 x 40 (one sees
    nothing); depth images: smooth surfaces through the cloud, 10 % zeros, NaN, negative and +inf pixels; owners -1 .. 2."""
    rng = np.random.default_rng(201)
    Q, H, W = 5003, 30, 40
    pts = np.stack([rng.uniform(-1, 1, Q), rng.uniform(-0.8, 0.8, Q), rng.uniform(1, 3, Q)], axis=1).astype(np.float32)
    poses = render_ref.case_posed()['poses']
    rr, cc = np.mgrid[0:H, 0:W]
    depth = np.stack([2.4 + 0.8 * np.sin(rr / 5.0) * np.cos(cc / 6.0), 0.5 + 0.3 * np.sin(rr / 4.0 + cc / 7.0),
                      2.0 + 0.0 * rr]).astype(np.float32)
    _spoil(depth, rng)
    return dict(points=pts, K=camera(24.0, 23.0, 19.7, 15.2), poses=poses, depth=depth, tol=0.05,
                owner=rng.integers(-1, 3, Q).astype(np.int32), view_owner=np.arange(3, dtype=np.int32))


THRESHOLD_TOL = 0.25


def case_thresholds():
    """Identity pose, 20 x 24, D = 2 and tol = 0.25 (b = 0.5, all exact).  Three depth images A, B, C to be used as single views; returns
    the case and ``expect``: {(view name, window): {point: class}} written by hand."""
    K = camera(16.0, 16.0, 8.5, 7.5)
    H, W = 20, 24
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    up, down = np.nextafter(np.float32(2.5), inf), np.nextafter(np.float32(1.5), -inf)

    def at(c, r, z):                                       # the point in the middle of pixel (r, c) at depth z: sums of dyadic numbers
        return [(c + 0.5 - 8.5) / 16.0 * z, (r + 0.5 - 7.5) / 16.0 * z, z]
    pts = np.array([[0.1, 0.1, 2.5],                       # 0  |2.5 - 2| = b: agrees
                    [0.1, 0.1, up],                        # 1  one float beyond: behind
                    [0.1, 0.1, 1.5],                       # 2  agrees
                    [0.1, 0.1, down],                      # 3  one float below D - b: in front
                    [-1.0625, 0.1, 2.0],                   # 4  u = 0 exactly: seen
                    [1.9375, 0.1, 2.0],                    # 5  u = W: not seen
                    [0.0, 0.0, np.float32(Z_MIN)],         # 6  z = z_min: not seen
                    [nan, 0.2, 2.0], [0.2, nan, 2.0], [0.2, 0.2, nan], [inf, 0.2, 2.0], [0.2, -inf, 2.0],    # 7 .. 11
                    [0.3, 0.3, inf],                       # 12 z = inf lands on (cy, cx) behind everything
                    at(0, 0, 2.0),                         # 13 the corner pixel
                    at(12, 10, 2.0),                       # 14 only a neighbour is valid
                    at(5, 5, 2.0)], np.float32)            # 15 between a nearer and a farther surface
    A = np.full((H, W), 2.0, np.float32)
    B = np.zeros((H, W), np.float32)
    B[2, 2] = B[0, 3] = B[3, 0] = B[3, 3] = 2.0            # (2, 2) is in the corner's clipped 3 x 3 at window 2; the others are outside
    B[10, 13] = 2.0
    C = np.zeros((H, W), np.float32)
    C[5, 5], C[5, 6] = 1.0, 4.0
    unseen = {k: UNSEEN for k in (5, 6, 7, 8, 9, 10, 11)}
    expect = {('A', 1): {**unseen, 0: AGREE, 1: BEHIND, 2: AGREE, 3: IN_FRONT, 4: AGREE, 12: BEHIND, 13: AGREE, 14: AGREE, 15: AGREE},
              ('B', 2): {**unseen, 13: AGREE, 14: AGREE}, ('B', 1): {**unseen, 13: UNSEEN, 14: AGREE},
              ('B', 0): {**unseen, 13: UNSEEN, 14: UNSEEN},
              ('C', 1): {**unseen, 15: BEHIND}, ('C', 0): {**unseen, 15: BEHIND}}
    eye = np.eye(4, dtype=np.float32)
    return dict(points=pts, K=K, poses=eye[None], depth=dict(A=A, B=B, C=C), tol=THRESHOLD_TOL), expect


def case_owners():
    """Q = 600 in front of four slightly shifted views of 16 x 20 whose depth images are valid everywhere (every pair in the image is one
    of the three classes); owners -1 .. 3."""
    rng = np.random.default_rng(202)
    Q, H, W = 600, 16, 20
    z = rng.uniform(1.2, 3.0, Q)
    pts = np.stack([rng.uniform(-0.45, 0.45, Q) * z, rng.uniform(-0.4, 0.4, Q) * z, z], axis=1).astype(np.float32)
    poses = np.stack([pose_of([0.01 * k, -0.02 * k, 0.005 * k], [0.03 * k, -0.02 * k, 0.01 * k]) for k in range(1, 5)])
    depth = rng.uniform(1.5, 2.8, (4, H, W)).astype(np.float32)
    return dict(points=pts, K=camera(16.0, 15.0, 10.2, 8.1), poses=poses, depth=depth, tol=0.05, owner=rng.integers(-1, 4, Q).astype(np.int32))


def case_many_views(V=70):
    """Q = 300 against V views of 8 x 10: more views than one workgroup takes."""
    rng = np.random.default_rng(203)
    Q, H, W = 300, 8, 10
    z = rng.uniform(1.0, 3.0, Q)
    pts = np.stack([rng.uniform(-0.6, 0.6, Q) * z, rng.uniform(-0.5, 0.5, Q) * z, z], axis=1).astype(np.float32)
    poses = np.stack([pose_of(0.05 * rng.standard_normal(3), 0.1 * rng.standard_normal(3)) for _ in range(V)])
    depth = _spoil(rng.uniform(1.0, 3.0, (V, H, W)).astype(np.float32), rng)
    return dict(points=pts, K=camera(8.0, 7.5, 5.1, 4.2), poses=poses, depth=depth, tol=0.05,
                owner=rng.integers(-1, V, Q).astype(np.int32), view_owner=np.arange(V, dtype=np.int32))


def case_collide():
    """map_render_ref.case_collide's 70 001 points into two views of 24 x 32 (the identity and a small motion): indices beyond 65 535,
    about 90 points per pixel."""
    rng = np.random.default_rng(204)
    c = render_ref.case_collide()
    H, W = c['H'], c['W']
    rr, cc = np.mgrid[0:H, 0:W]
    depth = np.stack([2.2 + 1.2 * np.sin(rr / 4.0) * np.cos(cc / 5.0), 2.0 + 1.0 * np.cos(rr / 6.0 + cc / 3.0)]).astype(np.float32)
    _spoil(depth, rng)
    poses = np.stack([np.eye(4, dtype=np.float32), pose_of([0.02, -0.03, 0.01], [0.05, 0.02, -0.1])])
    return dict(points=c['points'], K=c['K'], poses=poses, depth=depth, tol=0.05)


RANDOM_CASES = dict(posed=case_posed, owners=case_owners, many_views=case_many_views, collide=case_collide)


def case_keyframes():
    """Two 37 x 53 keyframes (N = 5 and 3) as arrays for ``KeyFrame``: nested and overlapping masks and one empty segment each.  In the
    first, segment 3 repeats segment 0 on a sub-rectangle with the same log-depths, keypoint value and kld: its points duplicate
    segment 0's z bit for bit, and the higher table index wins.  One kld is NaN and one is huge (z = inf): their points are skipped."""
    H, W = 37, 53
    rng = np.random.default_rng(205)
    out = []
    for k, N in enumerate((5, 3)):
        masks = np.zeros((N, H, W), bool)
        L = (0.3 * rng.standard_normal((N, H, W)) + 0.8).astype(np.float32)
        kld = (0.2 * rng.standard_normal(N) + 0.5).astype(np.float32)
        keyp = np.zeros((N, 2), np.int64)
        if k == 0:
            masks[0, 3:30, 4:40] = True
            masks[1, 10:20, 12:25] = True                  # nested in segment 0
            masks[2, 25:36, 30:52] = True                  # overlaps segment 0
            masks[3, 5:15, 6:30] = True                    # the duplicate of segment 0 there (segment 4 is empty)
            L[3] = L[0]
            kld[3] = kld[0]
            keyp[:4] = [(8, 10), (15, 18), (30, 45), (8, 10)]
            kld[1] = np.nan
        else:
            masks[0, 0:37, 0:20] = True
            masks[2, 12:30, 10:53] = True                  # overlaps segment 0 (segment 1 is empty)
            keyp[[0, 2]] = [(5, 5), (20, 40)]
            kld[0] = 200.0
            masks[2, 0, 52] = masks[2, 36, 52] = True      # the corners of the last column
        L = L * masks
        keypoints = np.stack([2.0 * keyp[:, 0] / (H - 1) - 1.0, 2.0 * keyp[:, 1] / (W - 1) - 1.0], axis=1).astype(np.float32)
        image = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
        K = np.array([[0.9 * W, 0, 0.5 * W - 0.25], [0, 0.95 * W, 0.5 * H + 0.5], [0, 0, 1]], np.float32)
        out.append(dict(masks=masks, L=L, keypoints=keypoints, kld=kld, image=image, K=K))
    return out


_CACHE = {}


def reference(name, window):
    """(case, classes (Q,V), ambiguous (Q,V)) of a random case at ``window``, made once per process and shared: nobody writes to them."""
    key = (name, window)
    if key not in _CACHE:
        c = RANDOM_CASES[name]()
        cls = classes(c['points'], c['K'], c['poses'], c['depth'], c.get('owner'), c.get('view_owner'), c['tol'], window)
        amb = ambiguous(c['points'], c['K'], c['poses'], c['depth'], c['tol'], window)
        _CACHE[key] = (c, cls, amb)
    return _CACHE[key]
