"""NumPy float64 statements of the map views (include/sp_hip.h: sp_render_views, sp_depth_lift), independent of the kernels: the
projection as tool/viz.py:163-178 forms it, the winner of every pixel by an explicit loop over the points, the image conversion, the
depth lift as Open3D documents create_from_depth_image -- and the two masks of pixels where a result may legitimately depend on the
last bit of a float64 sum.  The inputs of every device case are made here too, so that the host tests can check them.

Position taint: a point whose u or v lies within DELTA px of a pixel edge (an integer; the image border is one) may land on either side
when the float64 sums are formed in another order; every pixel it could reach is marked.  With the identity pose there is no sum at all
-- the arithmetic is NumPy's, operation for operation -- so the device tests use this mask for posed views only.

Depth-tie taint (mode 1): the pixel's two nearest kept points have float64 z within 5e-7 relative of each other, while neither their
float32(z) nor their coordinates are identical.  Equal float32(z) is decided by the index and exact duplicates are the same point: both
are unambiguous."""
import hashlib

import numpy as np

DELTA = 1e-6
Z_MIN = 1e-6
TIE_RTOL = 5e-7


def is_identity(pose):
    return pose is None or np.array_equal(np.asarray(pose)[:3], np.eye(4)[:3])


def camera_points(points, pose=None, order=0):
    """p_c = R^T (p - t) in float64 from float32 inputs, every operation rounded on its own; ``order`` picks the order of the
    three-term sums: 0 (a + b) + c [the kernel's], 1 a + (b + c), 2 (a + c) + b.  The identity pose leaves the points untouched."""
    p = np.asarray(points, np.float32).astype(np.float64)
    if is_identity(pose):
        return p[:, 0], p[:, 1], p[:, 2]
    T = np.asarray(pose, np.float32).astype(np.float64)
    d = [p[:, k] - T[k, 3] for k in range(3)]
    out = []
    with np.errstate(invalid='ignore', over='ignore'):
        for r in range(3):
            a, b, c = T[0, r] * d[0], T[1, r] * d[1], T[2, r] * d[2]
            out.append(((a + b) + c, a + (b + c), (a + c) + b)[order])
    return tuple(out)


def project(points, K, pose=None, order=0):
    """tool/viz.py:163-178 in float64: u = x fx / z + cx, v = y fy / z + cy; returns u, v, z."""
    K = np.asarray(K, np.float32).astype(np.float64)
    x, y, z = camera_points(points, pose, order)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        u = x * K[0, 0] / z + K[0, 2]
        v = y * K[1, 1] / z + K[1, 2]
    return u, v, z


def colour_u8(colours):
    """trunc(c * 255) from the exact float64 product, clamped to 0 .. 255, NaN -> 0."""
    p = np.asarray(colours, np.float32).astype(np.float64) * 255.0
    with np.errstate(invalid='ignore'):
        p = np.where(p > 0.0, np.minimum(p, 255.0), 0.0)
    return np.trunc(p).astype(np.uint8)


def render(points, colours, K, pose, H, W, mode, z_min=Z_MIN):
    """One view.  Returns image (H,W,3) uint8, depth (H,W) float32, index (H,W) int32.  The winner of a pixel by a loop over the kept
    points in ascending index: mode 0 -- every kept point overwrites; mode 1 -- z > z_min, and a point takes the pixel when its
    float32(z) is smaller than or EQUAL to the holder's (it has the higher index)."""
    u, v, z = project(points, K, pose)
    with np.errstate(invalid='ignore'):
        keep = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        if mode == 1:
            keep &= z > np.float64(np.float32(z_min))
    zf = z.astype(np.float32)
    index = np.full((H, W), -1, np.int32)
    best = np.zeros((H, W), np.float32)
    for i in np.nonzero(keep)[0]:
        r, c = int(v[i]), int(u[i])
        if mode == 0 or index[r, c] < 0 or zf[i] <= best[r, c]:
            index[r, c], best[r, c] = i, zf[i]
    hit = index >= 0
    depth = np.where(hit, best, np.float32(0)).astype(np.float32)
    image = np.zeros((H, W, 3), np.uint8)
    if colours is not None:
        image[hit] = colour_u8(colours)[index[hit]]
    return image, depth, index


def position_taint(points, K, pose, H, W, delta=DELTA):
    """(H,W) bool: every pixel a point within ``delta`` px of a pixel edge (or within 1e-9 of z = z_min) could reach."""
    u, v, z = project(points, K, pose)
    taint = np.zeros((H, W), bool)
    with np.errstate(invalid='ignore'):
        near = (np.abs(u - np.round(u)) <= delta) | (np.abs(v - np.round(v)) <= delta) | (np.abs(z - Z_MIN) <= 1e-9)
        amb = np.isfinite(u) & np.isfinite(v) & near & (u > -1) & (u < W + 1) & (v > -1) & (v < H + 1)
    for i in np.nonzero(amb)[0]:
        rows = {int(np.floor(v[i] - delta)), int(np.floor(v[i] + delta))}
        cols = {int(np.floor(u[i] - delta)), int(np.floor(u[i] + delta))}
        for r in rows:
            for c in cols:
                if 0 <= r < H and 0 <= c < W:
                    taint[r, c] = True
    return taint


def depth_tie_taint(points, K, pose, H, W, z_min=Z_MIN, rtol=TIE_RTOL):
    """(H,W) bool, mode 1: the two nearest kept points of the pixel (by float64 z) agree within ``rtol`` relative while neither their
    float32(z) nor their coordinates are identical."""
    u, v, z = project(points, K, pose)
    pts = np.asarray(points, np.float32)
    with np.errstate(invalid='ignore'):
        keep = (u >= 0) & (u < W) & (v >= 0) & (v < H) & (z > np.float64(np.float32(z_min)))
    first = np.full((H, W), -1, np.int64)
    second = np.full((H, W), -1, np.int64)
    for i in np.nonzero(keep)[0]:
        r, c = int(v[i]), int(u[i])
        a, b = first[r, c], second[r, c]
        if a < 0 or z[i] <= z[a]:
            first[r, c], second[r, c] = i, a
        elif b < 0 or z[i] <= z[b]:
            second[r, c] = i
    taint = np.zeros((H, W), bool)
    for r, c in zip(*np.nonzero(second >= 0)):
        a, b = first[r, c], second[r, c]
        close = abs(z[a] - z[b]) <= rtol * max(abs(z[a]), abs(z[b]))
        same_f32 = np.float32(z[a]) == np.float32(z[b])
        same_point = np.array_equal(pts[a], pts[b])
        taint[r, c] = close and not same_f32 and not same_point
    return taint


def lift(depth, K, pose=None, image=None, depth_trunc=100.0):
    """sp_depth_lift in float64: depth (B,H,W) float32, K (B,3,3), pose (B,4,4) or None, image (B,3,H,W) or None.  Returns dict(points
    (n,3) float64, colours (n,3) float32 or None, pixel (n,) int32, counts (B,) int32, offsets (B+1,) int64), rows in row-major order,
    image after image."""
    depth = np.asarray(depth, np.float32)
    B, H, W = depth.shape
    pts, cols, pix, counts = [], [], [], []
    for b in range(B):
        d32 = depth[b]
        with np.errstate(invalid='ignore'):
            valid = (d32 > 0) & (d32 <= np.float32(depth_trunc))
        r, c = np.nonzero(valid)                                     # row-major
        Kb = np.asarray(K[b], np.float32).astype(np.float64)
        d = d32[valid].astype(np.float64)
        x = (c.astype(np.float64) - Kb[0, 2]) * d / Kb[0, 0]
        y = (r.astype(np.float64) - Kb[1, 2]) * d / Kb[1, 1]
        p = np.stack([x, y, d], axis=1)
        if pose is not None:
            T = np.asarray(pose[b], np.float32).astype(np.float64)
            p = np.stack([((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * d) + T[k, 3] for k in range(3)], axis=1)
        pts.append(p)
        pix.append((r * W + c).astype(np.int32))
        counts.append(len(r))
        if image is not None:
            cols.append(np.asarray(image[b], np.float32)[:, r, c].T)
    return dict(points=np.concatenate(pts), colours=np.concatenate(cols) if image is not None else None, pixel=np.concatenate(pix),
                counts=np.asarray(counts, np.int32), offsets=np.concatenate(([0], np.cumsum(counts))).astype(np.int64))


# ---- the inputs of the device cases ------------------------------------------------------------------------------------------------
def camera(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def pose_of(rotvec, t):
    """Camera-to-world (4,4) float32 from a rotation vector (Rodrigues) and a translation."""
    w = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(w)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T.astype(np.float32)


def case_golden0():
    """Q = 5003 (not a multiple of 256, 20 workgroups) into 37 x 53; z over [-0.5, 4]: points behind the camera and near z = 0."""
    rng = np.random.default_rng(101)
    Q = 5003
    pts = np.stack([rng.uniform(-2.0, 2.0, Q), rng.uniform(-1.5, 1.5, Q), rng.uniform(-0.5, 4.0, Q)], axis=1).astype(np.float32)
    cols = rng.uniform(0.0, 1.0, (Q, 3)).astype(np.float32)
    cols[7], cols[11] = 1.0, 0.0
    return dict(points=pts, colours=cols, K=camera(41.5, 39.25, 26.3, 18.1), H=37, W=53)


def case_collide():
    """Q = 70 001 into 24 x 32: about 90 points per pixel, indices beyond 65 535."""
    rng = np.random.default_rng(102)
    Q = 70001
    z = rng.uniform(0.5, 4.0, Q)
    pts = np.stack([rng.uniform(-0.5, 0.5, Q) * z, rng.uniform(-0.5, 0.5, Q) * z, z], axis=1).astype(np.float32)
    cols = rng.uniform(0.0, 1.0, (Q, 3)).astype(np.float32)
    return dict(points=pts, colours=cols, K=camera(30.0, 22.0, 16.2, 12.4), H=24, W=32)


GOLDEN_CASES = dict(golden0=case_golden0, collide=case_collide)


def digest(case):
    h = hashlib.sha256()
    for k in ('points', 'colours', 'K'):
        h.update(np.ascontiguousarray(case[k]).tobytes())
    return h.hexdigest()


def case_duplicates():
    """Mode 1: 600 points into 16 x 20 seen through a pure translation t = (0, 0, -7) (so z_c = z + 7 is a float64 sum); rows 500..549
    repeat rows 0..49 with other colours (exact duplicates at low and high indices); rows 550 / 551 sit alone in pixel (1, 1) with
    float64 z_c = 9 and 9 + 2^-22, one float32(z) = 9: the index decides.  Returns the case and the pair's pixel."""
    rng = np.random.default_rng(103)
    K = camera(16.0, 16.0, 10.0, 8.0)
    z = rng.uniform(1.0, 3.0, 600)
    zc = z + 7.0
    pts = np.stack([rng.uniform(-0.3, 0.55, 600) * zc, rng.uniform(-0.3, 0.45, 600) * zc, z], axis=1).astype(np.float32)
    pts[500:550] = pts[:50]
    # the pair: camera-frame (x, y) = (-4.8, -3.6) at z_c = 9 -> u = 10 - 8.53 = 1.47, v = 8 - 6.4 = 1.6; nothing else may land there
    u, v, _ = project(pts, K, pose_of([0, 0, 0], [0, 0, -7]))
    crowd = (np.floor(u) == 1) & (np.floor(v) == 1)
    pts[crowd, 0] += 3.0
    pts[550] = (-4.8, -3.6, 2.0)
    pts[551] = (-4.8, -3.6, np.float32(2.0) + np.float32(2.0 ** -22))
    cols = rng.uniform(0.0, 1.0, (600, 3)).astype(np.float32)
    return dict(points=pts, colours=cols, K=K, H=16, W=20, poses=pose_of([0, 0, 0], [0, 0, -7])[None]), (1, 1)


def case_posed():
    """Q = 3001 in the box [-1, 1] x [-0.8, 0.8] x [1, 3], three views of 30 x 40: one looks at the cloud, one sits at its centre turned
    by 90 degrees about y (the points with x < 0 are behind it), one stands 100 units aside and sees nothing in either mode."""
    rng = np.random.default_rng(104)
    Q = 3001
    pts = np.stack([rng.uniform(-1, 1, Q), rng.uniform(-0.8, 0.8, Q), rng.uniform(1, 3, Q)], axis=1).astype(np.float32)
    cols = rng.uniform(0.0, 1.0, (Q, 3)).astype(np.float32)
    poses = np.stack([pose_of([0.05, -0.08, 0.03], [0.1, -0.05, -0.4]), pose_of([0, np.pi / 2, 0], [0.013, 0.021, 2.0]),
                      pose_of([0, 0, 0], [100.0, 0, 0])])
    return dict(points=pts, colours=cols, K=camera(24.0, 23.0, 19.7, 15.2), H=30, W=40, poses=poses)


def case_edges():
    """20 x 24, identity pose: a point exactly on u = 0 (kept), one on u = W (dropped), NaN and inf coordinates, a NaN colour, and a point
    at z = inf (the reference keeps it, at (cy, cx))."""
    K = camera(16.0, 16.0, 8.5, 7.5)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    pts = np.array([[-1.0625, 0.1, 2.0],          # u = -8.5 + 8.5 = 0 exactly: kept, column 0
                    [1.9375, 0.1, 2.0],           # u = 15.5 + 8.5 = 24 = W: dropped
                    [nan, 0.2, 2.0], [0.2, nan, 2.0], [0.2, 0.2, nan],
                    [inf, 0.2, 2.0], [0.2, -inf, 2.0],
                    [0.3, 0.3, inf],              # u = cx, v = cy
                    [0.5, 0.5, 2.0],              # NaN colour
                    [0.25, -0.25, 1.0], [0.25, -0.25, -1.0]], np.float32)
    cols = np.linspace(0.05, 0.95, pts.size, dtype=np.float32).reshape(-1, 3)
    cols[8] = (nan, 0.5, nan)
    return dict(points=pts, colours=cols, K=K, H=20, W=24)


def lift_inputs(B, H, W, seed):
    """Depths with 0, negatives, NaN and values above depth_trunc = 100 scattered in; colours; cameras; poses."""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(0.5, 4.0, (B, H, W)).astype(np.float32)
    kind = rng.integers(0, 10, (B, H, W))
    depth[kind == 0] = 0.0
    depth[kind == 1] = -1.5
    depth[kind == 2] = np.nan
    depth[kind == 3] = 100.5
    depth[0, 0, 0], depth[0, 0, 1] = 100.0, np.inf                 # exactly depth_trunc is valid
    image = rng.uniform(0.0, 1.0, (B, 3, H, W)).astype(np.float32)
    K = np.stack([camera(20.0 + b, 21.0 + b, W / 2 - 0.3 * b, H / 2 + 0.2 * b) for b in range(B)])
    poses = np.stack([pose_of(0.2 * rng.standard_normal(3), rng.uniform(-1, 1, 3)) for _ in range(B)])
    return depth, K, poses, image


def lift_case_small():
    """B = 3 images of 19 x 23: mixed, ALL invalid, ALL valid."""
    depth, K, poses, image = lift_inputs(3, 19, 23, 105)
    depth[1] = np.where(np.arange(19 * 23).reshape(19, 23) % 2 == 0, 0.0, np.nan).astype(np.float32)
    depth[2] = np.abs(np.nan_to_num(depth[2], nan=1.0)) % 50 + 0.25
    return depth, K, poses, image


def lift_case_single():
    """One image of 64 x 80 (20 blocks of 256 pixels)."""
    return lift_inputs(1, 64, 80, 106)


def lift_case_blocks():
    """B = 3 images of 150 x 150: 88 blocks of 256 pixels per image, 264 in all -- more than the 256 threads of the block-count scan, so
    every scan thread takes two blocks; images 1 and 2 start at blocks 88 and 176, the FIRST of a thread's pair."""
    return lift_inputs(3, 150, 150, 108)


def lift_case_blocks_odd():
    """B = 3 images of 149 x 149: 87 blocks per image, 261 in all, two per scan thread; image 1 starts at block 87, the SECOND of a
    thread's pair (an image boundary inside a thread's range), image 2 at block 174, the first of one."""
    return lift_inputs(3, 149, 149, 109)
