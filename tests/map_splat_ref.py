"""NumPy float64 statements of the footprint render and the image score (include/sp_hip.h: sp_render_splats, sp_image_metrics),
independent of the kernels: the projection of tests/map_render_ref.py, the half-widths and the rectangle of every point, the winner of
every pixel by an explicit loop over the points and their rectangles, the integer sums of the image score -- and the two ambiguity masks
of map_render_ref, generalised from a point's pixel to a footprint's rectangle.  The inputs of every device case are made here too.

Position taint: a kept (or nearly kept) point one of whose four edges u -+ ru, v -+ rv lies within DELTA px of an integer (a pixel
edge; the image border is one), or whose z lies within 1e-9 of z_min, may cover another set of pixels when the float64 sums are formed
in another order; every pixel of its rectangle widened by DELTA is marked.
Depth-tie taint: the two nearest points covering a pixel have float64 z within 5e-7 relative of each other while neither their
float32(z) nor their coordinates are identical."""
import numpy as np

import map_render_ref as base
from map_render_ref import DELTA, TIE_RTOL, Z_MIN, camera, colour_u8, is_identity, pose_of, project  # noqa: F401  (the cases' tools)


def footprints(points, radii, K, pose, max_px, order=0):
    """u, v, z and the half-widths ru, rv in pixels: (r fx) / z, (r fy) / z in float64; not >= 0 -> 0, else min(., max_px)."""
    Kd = np.asarray(K, np.float32).astype(np.float64)
    u, v, z = project(points, K, pose, order)
    r = np.asarray(radii, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ru, rv = (r * Kd[0, 0]) / z, (r * Kd[1, 1]) / z
        ru = np.where(ru >= 0, np.minimum(ru, float(max_px)), 0.0)
        rv = np.where(rv >= 0, np.minimum(rv, float(max_px)), 0.0)
    return u, v, z, ru, rv


def kept(u, v, z, ru, rv, H, W, z_min=Z_MIN):
    with np.errstate(invalid='ignore'):
        return (np.isfinite(u) & np.isfinite(v) & (z > np.float64(np.float32(z_min)))
                & (u + ru >= 0) & (u - ru < W) & (v + rv >= 0) & (v - rv < H))


def rectangle(u, v, ru, rv, H, W, widen=0.0):
    """(r0, r1, c0, c1), inclusive, of ONE kept point: clamped in float64, then converted."""
    c0, c1 = int(max(np.floor(u - ru - widen), 0.0)), int(min(np.floor(u + ru + widen), W - 1.0))
    r0, r1 = int(max(np.floor(v - rv - widen), 0.0)), int(min(np.floor(v + rv + widen), H - 1.0))
    return r0, r1, c0, c1


def render(points, colours, radii, K, pose, H, W, max_px, z_min=Z_MIN):
    """One view.  Returns image (H,W,3) uint8, depth (H,W) float32, index (H,W) int32.  A loop over the kept points in ascending index
    and over the pixels of each one's rectangle: a point takes a pixel that is empty or whose holder's float32(z) is larger than or
    EQUAL to its own (it has the higher index)."""
    u, v, z, ru, rv = footprints(points, radii, K, pose, max_px)
    zf = z.astype(np.float32)
    index = np.full((H, W), -1, np.int32)
    best = np.zeros((H, W), np.float32)
    for i in np.nonzero(kept(u, v, z, ru, rv, H, W, z_min))[0]:
        r0, r1, c0, c1 = rectangle(u[i], v[i], ru[i], rv[i], H, W)
        for r in range(r0, r1 + 1):
            for c in range(c0, c1 + 1):
                if index[r, c] < 0 or zf[i] <= best[r, c]:
                    index[r, c], best[r, c] = i, zf[i]
    hit = index >= 0
    depth = np.where(hit, best, np.float32(0)).astype(np.float32)
    image = np.zeros((H, W, 3), np.uint8)
    if colours is not None:
        image[hit] = colour_u8(colours)[index[hit]]
    return image, depth, index


def triples(points, radii, K, pose, H, W, max_px, z_min=Z_MIN):
    """The number of covered (point, pixel) pairs of one view, and how many points sit at the cap in either direction."""
    u, v, z, ru, rv = footprints(points, radii, K, pose, max_px)
    keep = kept(u, v, z, ru, rv, H, W, z_min)
    n = 0
    for i in np.nonzero(keep)[0]:
        r0, r1, c0, c1 = rectangle(u[i], v[i], ru[i], rv[i], H, W)
        n += (r1 - r0 + 1) * (c1 - c0 + 1)
    return n, int((keep & ((ru == max_px) | (rv == max_px))).sum())


def position_taint(points, radii, K, pose, H, W, max_px, delta=DELTA):
    """(H,W) bool: every pixel of the rectangle, widened by ``delta``, of a point with an edge within ``delta`` px of an integer or
    with z within 1e-9 of z_min."""
    u, v, z, ru, rv = footprints(points, radii, K, pose, max_px)
    taint = np.zeros((H, W), bool)
    with np.errstate(invalid='ignore'):
        near = np.abs(z - Z_MIN) <= 1e-9
        for e in (u - ru, u + ru, v - rv, v + rv):
            near |= np.abs(e - np.round(e)) <= delta
        amb = (np.isfinite(u) & np.isfinite(v) & near & (z > Z_MIN - 1e-9)
               & (u + ru > -1) & (u - ru < W + 1) & (v + rv > -1) & (v - rv < H + 1))
    for i in np.nonzero(amb)[0]:
        r0, r1, c0, c1 = rectangle(u[i], v[i], ru[i], rv[i], H, W, widen=delta)
        taint[r0:r1 + 1, c0:c1 + 1] = True
    return taint


def depth_tie_taint(points, radii, K, pose, H, W, max_px, z_min=Z_MIN, rtol=TIE_RTOL):
    """(H,W) bool: the two nearest points covering the pixel (by float64 z) agree within ``rtol`` relative while neither their
    float32(z) nor their coordinates are identical."""
    u, v, z, ru, rv = footprints(points, radii, K, pose, max_px)
    pts = np.asarray(points, np.float32)
    first = np.full((H, W), -1, np.int64)
    second = np.full((H, W), -1, np.int64)
    z1 = np.full((H, W), np.inf)
    z2 = np.full((H, W), np.inf)
    for i in np.nonzero(kept(u, v, z, ru, rv, H, W, z_min))[0]:
        r0, r1, c0, c1 = rectangle(u[i], v[i], ru[i], rv[i], H, W)
        sl = (slice(r0, r1 + 1), slice(c0, c1 + 1))
        a, b, za, zb = first[sl], second[sl], z1[sl], z2[sl]
        to_first = (a < 0) | (z[i] <= za)
        to_second = ~to_first & ((b < 0) | (z[i] <= zb))
        second[sl], z2[sl] = np.where(to_first, a, np.where(to_second, i, b)), np.where(to_first, za, np.where(to_second, z[i], zb))
        first[sl], z1[sl] = np.where(to_first, i, a), np.where(to_first, z[i], za)
    taint = np.zeros((H, W), bool)
    for r, c in zip(*np.nonzero(second >= 0)):
        a, b = first[r, c], second[r, c]
        close = abs(z[a] - z[b]) <= rtol * max(abs(z[a]), abs(z[b]))
        same_f32 = np.float32(z[a]) == np.float32(z[b])
        same_point = np.array_equal(pts[a], pts[b])
        taint[r, c] = close and not same_f32 and not same_point
    return taint


def image_metrics(rendered, target, index):
    """sp_image_metrics with NumPy integers: rendered (V,H,W,3) uint8, target (V,3,H,W) float32, index (V,H,W) int32 -> (V,3) int64:
    n, sum |a - b|, sum (a - b)^2 over the pixels with index >= 0 and their three channels."""
    a = np.asarray(rendered).astype(np.int64)
    b = colour_u8(np.asarray(target, np.float32).transpose(0, 2, 3, 1)).astype(np.int64)
    out = np.zeros((a.shape[0], 3), np.int64)
    for k in range(a.shape[0]):
        m = np.asarray(index[k]) >= 0
        d = np.abs(a[k][m] - b[k][m])
        out[k] = int(m.sum()), int(d.sum()), int((d * d).sum())
    return out


# ---- the inputs of the device cases ------------------------------------------------------------------------------------------------
def case_splat_posed():
    """case_posed() (3001 points, three views of 30 x 40) with radii in [0, 0.12), every 7th exactly 0; max_px 3."""
    c = dict(base.case_posed())
    radii = np.random.default_rng(201).uniform(0, 0.12, len(c['points'])).astype(np.float32)
    radii[::7] = 0.0
    c.update(radii=radii, max_px=3)
    return c


def case_splat_collide():
    """case_collide() (70 001 points into 24 x 32) with radii 0.012 z (about a third of a pixel to either side from the identity pose),
    seen from the identity pose and from a camera 0.3 behind it, slightly turned; max_px 2."""
    c = dict(base.case_collide())
    radii = (np.float32(0.012) * c['points'][:, 2]).astype(np.float32)
    poses = np.stack([np.eye(4, dtype=np.float32), pose_of([0.01, 0.02, -0.015], [0.02, -0.01, -0.3])])
    c.update(radii=radii, max_px=2, poses=poses)
    return c


def case_splat_views17():
    """The first 300 points of case_posed() into 17 views of 30 x 40: one view more than the kernel stages at a time; max_px 3."""
    p = base.case_posed()
    rng = np.random.default_rng(202)
    radii = rng.uniform(0, 0.12, 300).astype(np.float32)
    poses = np.stack([pose_of(0.03 * rng.standard_normal(3), np.array([0.1, -0.05, -0.4]) + 0.05 * rng.standard_normal(3)) for _ in range(17)])
    return dict(points=p['points'][:300], colours=p['colours'][:300], K=p['K'], H=30, W=40, poses=poses, radii=radii, max_px=3)


EDGE_ROWS = dict(reaches=0, misses=1, nan_radius=2, negative_radius=3, inf_radius=4, z_inf=5, corner=6, below_z_min=7, near=8, nan_point=9,
                 zero_radius=10)


def case_splat_edges():
    """20 x 24, identity pose, K = (16, 16, 8.5, 7.5), max_px 3: eleven constructed points (EDGE_ROWS names their rows)."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    rows = [([-1.125, 0.1, 2.0], 0.125),          # u = -0.5, ru = 1: the square reaches column 0 (rows 7..9)
            ([-1.25, 0.85, 2.0], 0.125),          # u = -1.5, ru = 1: u + ru = -0.5, it does not reach
            ([-0.625, 0.625, 2.0], nan),          # a point at (12, 3)
            ([-0.25, 0.625, 2.0], -0.5),          # a point at (12, 6)
            ([-0.5, -0.375, 2.0], inf),           # u = v = 4.5: the square at the cap, rows and columns 1..7
            ([0.3, 0.3, inf], 0.1),               # half-width 0, a point at (cy, cx) = (7, 8) with depth inf
            ([1.75, 1.375, 2.0], 1e9),            # u = 22.5, v = 18.5: the cap's square clipped to columns 19..23, rows 15..19
            ([0.0, 0.0, 5e-7], 0.1),              # z below z_min: dropped (it would win (7, 8))
            ([0.00375, -0.001875, 0.01], 0.01),   # u = 14.5, v = 4.5, ru = 16 -> the cap: rows 1..7, columns 11..17
            ([nan, 0.2, 2.0], 0.1),               # dropped
            ([0.125, 0.625, 2.0], 0.0)]           # a point at (12, 9)
    pts = np.array([p for p, _ in rows], np.float32)
    radii = np.array([r for _, r in rows], np.float32)
    cols = np.linspace(0.05, 0.95, pts.size, dtype=np.float32).reshape(-1, 3)
    return dict(points=pts, colours=cols, K=camera(16.0, 16.0, 8.5, 7.5), H=20, W=24, radii=radii, max_px=3)


CASES = dict(splat_posed=case_splat_posed, splat_collide=case_splat_collide, splat_views17=case_splat_views17, splat_edges=case_splat_edges)


def case_plane(footprint):
    """A 48 x 64 plane gt = 1.5 + 0.01 c + 0.015 r sampled at every second pixel in both directions, each sample lifted at its integer
    coordinate (float64, rounded to float32) with radius footprint d / (2 fx); ``K_mid`` renders it back with every point in the
    middle of its pixel.  ``bound``: a winner lies within floor(footprint / 2 + 0.5) pixels per axis, 0.025 of depth per pixel; 1e-6
    for the float32 rounding of depths below 4."""
    H, W = 48, 64
    K = camera(52.0, 50.0, 31.3, 23.6)
    Kd = K.astype(np.float64)
    rr, cc = np.mgrid[0:H, 0:W]
    gt = 1.5 + 0.01 * cc + 0.015 * rr
    r, c = rr[::2, ::2].reshape(-1), cc[::2, ::2].reshape(-1)
    d = gt[r, c]
    pts = np.stack([(c - Kd[0, 2]) * d / Kd[0, 0], (r - Kd[1, 2]) * d / Kd[1, 1], d], axis=1).astype(np.float32)
    radii = (footprint * d / (2.0 * Kd[0, 0])).astype(np.float32)
    K_mid = K.copy()
    K_mid[0, 2] += 0.5
    K_mid[1, 2] += 0.5
    cols = np.stack([c / 64.0, r / 48.0, 0.5 + 0 * d], axis=1).astype(np.float32)
    return dict(points=pts, colours=cols, radii=radii, K=K, K_mid=K_mid, H=H, W=W, gt=gt.astype(np.float32), max_px=4,
                bound=np.floor(footprint / 2 + 0.5) * 0.025 + 1e-6)


def metrics_inputs(V, H, W, seed):
    """Random uint8 views, an index with -1 in about a third of the pixels, a target in [-0.2, 1.2] with NaN scattered in."""
    rng = np.random.default_rng(seed)
    rendered = rng.integers(0, 256, (V, H, W, 3)).astype(np.uint8)
    index = np.where(rng.uniform(size=(V, H, W)) < 1 / 3, -1, rng.integers(0, 1000, (V, H, W))).astype(np.int32)
    target = rng.uniform(-0.2, 1.2, (V, 3, H, W)).astype(np.float32)
    target[rng.uniform(size=target.shape) < 0.02] = np.nan
    return rendered, target, index
