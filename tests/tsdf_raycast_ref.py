"""NumPy restatement of sp_tsdf_raycast's rule (include/sp_hip.h), written from the rule and not from the kernel: float64 from the float32
inputs, every operation on its own (NumPy contracts nothing), EVERY k of every ray marched -- no clipping against the volume --, vectorised
over the pixels of a view.  Test infrastructure only.  Also the volumes and cameras the host and device tests share."""
import functools

import numpy as np

import tsdf_ref
from map_render_ref import colour_u8, is_identity


def _f64(x):
    return np.float64(np.float32(x))


class Volume:
    """tsdf, weight (nz,ny,nx) float32, colour (nz,ny,nx,3) float32 or None, voxel, origin, min_weight: what the entry point is given."""

    def __init__(self, tsdf, weight, colour, voxel, origin, min_weight=1.0):
        assert tsdf.dtype == np.float32 and weight.dtype == np.float32 and tsdf.shape == weight.shape and (colour is None or colour.dtype == np.float32)
        self.tsdf, self.weight, self.colour = tsdf, weight, colour
        self.voxel, self.origin, self.min_weight = float(np.float32(voxel)), tuple(float(np.float32(o)) for o in origin), float(np.float32(min_weight))
        self.nz, self.ny, self.nx = tsdf.shape
        with np.errstate(invalid='ignore'):
            self.node_ok = (weight >= np.float32(min_weight)) & np.isfinite(tsdf)

    @property
    def dims(self):
        return (self.nx, self.ny, self.nz)


def world_points(K, pose, rows, cols, z):
    """p(z) of the pixels (rows, cols): xr = (col - cx) / fx, yr = (row - cy) / fy, q = (xr z, yr z, z), p_a = ((R_a0 q0 + R_a1 q1) + R_a2 q2)
    + t_a; an exact identity pose leaves p = q."""
    Kd, T = np.asarray(K, np.float32).astype(np.float64), np.asarray(pose, np.float32).astype(np.float64)
    with np.errstate(all='ignore'):
        xr = (cols.astype(np.float64) - Kd[0, 2]) / Kd[0, 0]
        yr = (rows.astype(np.float64) - Kd[1, 2]) / Kd[1, 1]
        q = (xr * z, yr * z, z + np.zeros_like(xr))
        if is_identity(pose):
            return q
        return tuple(((T[a, 0] * q[0] + T[a, 1] * q[1]) + T[a, 2] * q[2]) + T[a, 3] for a in range(3))


def _lerp3(corner, f):
    """corner[dz][dy][dx] (each (P,) float64), f = (fx, fy, fz): lerps a + f (b - a) along x, then y, then z."""
    x = [[corner[dz][dy][0] + f[0] * (corner[dz][dy][1] - corner[dz][dy][0]) for dy in (0, 1)] for dz in (0, 1)]
    y = [x[dz][0] + f[1] * (x[dz][1] - x[dz][0]) for dz in (0, 1)]
    return y[0] + f[2] * (y[1] - y[0])


def sample(vol, p, colour=False):
    """S(p) for (P,) world points p = (px, py, pz): valid (P,) bool, value (P,) float64 (0 where invalid), node (P,) int64 -- the lower
    node's linear index, -1 where the point has no cell --, and with ``colour`` the three channels C(p) as (P,3) float64."""
    n = (vol.nx, vol.ny, vol.nz)
    g, i, inside = [], [], np.ones(p[0].shape, bool)
    with np.errstate(all='ignore'):
        for a in range(3):
            ga = ((p[a] - _f64(vol.origin[a])) / _f64(vol.voxel)) - 0.5
            ia = np.floor(ga)
            inside &= np.isfinite(ga) & (ia >= 0) & (ia + 1 <= n[a] - 1)
            g.append(ga)
            i.append(ia)
    ii = [np.where(inside, ia, 0).astype(np.int64) for ia in i]
    f = [np.where(inside, ga - ia, 0.0) for ga, ia in zip(g, i)]
    ok = inside.copy()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                ok &= vol.node_ok[ii[2] + dz, ii[1] + dy, ii[0] + dx]
    corner = lambda field: [[[np.where(ok, field[ii[2] + dz, ii[1] + dy, ii[0] + dx], np.float32(0)).astype(np.float64) for dx in (0, 1)]
                             for dy in (0, 1)] for dz in (0, 1)]
    value = np.where(ok, _lerp3(corner(vol.tsdf), f), 0.0)
    node = np.where(inside, (ii[2] * vol.ny + ii[1]) * vol.nx + ii[0], -1)
    if not colour:
        return ok, value, node
    with np.errstate(all='ignore'):
        C = np.stack([_lerp3(corner(vol.colour[..., ch]), f) for ch in range(3)], axis=-1)
    return ok, value, node, C


def raycast_view(vol, K, pose, H, W, z_start, step, n_steps):
    """One view by the rule.  Returns depth (H,W) float32, normals (H,W,3) float32, image (H,W,3) uint8 (None for a volume without
    colour), index (H,W) int32 and the counts: hits, rays ended without a hit, hits with a NaN normal."""
    rows, cols = (a.reshape(-1) for a in np.meshgrid(np.arange(H), np.arange(W), indexing='ij'))
    P = H * W
    z0, st = _f64(z_start), _f64(step)
    running = np.ones(P, bool)                             # the ray has not ended
    prev_ok, prev_F = np.zeros(P, bool), np.zeros(P)
    hit, k_end, F_before, F_end = np.zeros(P, bool), np.full(P, -1, np.int64), np.zeros(P), np.zeros(P)
    for k in range(n_steps):                               # ALL k: nothing is skipped
        z = z0 + np.float64(k) * st
        ok, F, _ = sample(vol, world_points(K, pose, rows, cols, z))
        ends = running & ok & (F < 0.0)
        if k >= 1:
            now = ends & prev_ok & (prev_F >= 0.0)
            hit |= now
            F_before[now], F_end[now] = prev_F[now], F[now]
        k_end[ends] = k
        running &= ~ends
        prev_ok, prev_F = ok, F
    depth, index = np.zeros(P, np.float32), np.full(P, -1, np.int32)
    normals = np.full((P, 3), np.nan, np.float32)
    image = None if vol.colour is None else np.zeros((P, 3), np.uint8)
    nan_normals = 0
    if hit.any():
        h = np.flatnonzero(hit)
        r, c = rows[h], cols[h]
        t = F_before[h] / (F_before[h] - F_end[h])
        z_before = z0 + (k_end[h] - 1).astype(np.float64) * st
        z_at = z0 + k_end[h].astype(np.float64) * st
        zs = t * st + z_before
        depth[h] = zs.astype(np.float32)
        at_end = sample(vol, world_points(K, pose, r, c, z_at), colour=vol.colour is not None)
        before = sample(vol, world_points(K, pose, r, c, z_before), colour=vol.colour is not None)
        assert at_end[0].all() and before[0].all() and np.array_equal(at_end[1], F_end[h]) and np.array_equal(before[1], F_before[h])
        index[h] = at_end[2].astype(np.int32)
        if image is not None:
            with np.errstate(all='ignore'):
                image[h] = colour_u8((before[3] + t[:, None] * (at_end[3] - before[3])).astype(np.float32))
        p = world_points(K, pose, r, c, zs)
        hv = _f64(vol.voxel)
        g, all_ok = [], np.ones(len(h), bool)
        for a in range(3):
            plus = sample(vol, tuple(p[b] + hv if b == a else p[b] for b in range(3)))
            minus = sample(vol, tuple(p[b] - hv if b == a else p[b] for b in range(3)))
            all_ok &= plus[0] & minus[0]
            g.append(plus[1] - minus[1])
        with np.errstate(all='ignore'):
            length = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            good = all_ok & np.isfinite(length) & (length > 0.0)
            n = np.stack([ga / length for ga in g], axis=-1).astype(np.float32)
        normals[h] = np.where(good[:, None], n, np.float32(np.nan))
        nan_normals = int((~good).sum())
    counts = dict(hits=int(hit.sum()), ended_without_hit=int(((k_end >= 0) & ~hit).sum()), nan_normals=nan_normals)
    return (depth.reshape(H, W), normals.reshape(H, W, 3), None if image is None else image.reshape(H, W, 3), index.reshape(H, W), counts)


def raycast(vol, Ks, poses, H, W, z_start, step, n_steps):
    """V views: dict(depth (V,H,W), normals (V,H,W,3), image (V,H,W,3) or None, index (V,H,W), counts: a list of V dicts)."""
    views = [raycast_view(vol, Ks[v], poses[v], H, W, z_start, step, n_steps) for v in range(len(poses))]
    stack = lambda k: np.stack([v[k] for v in views])
    return dict(depth=stack(0), normals=stack(1), image=None if vol.colour is None else stack(2), index=stack(3), counts=[v[4] for v in views])


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------------
MAIN_STEPS = dict(z_start=0.0, step=0.125, n_steps=25)


@functools.lru_cache(maxsize=None)
def main_volume(colour=True):
    """tsdf_ref.case_main's three views integrated by its reference: 14 x 12 x 10 nodes of 1/8 around the slanted plane."""
    case = tsdf_ref.case_main()
    vol = tsdf_ref.reference(case, colour=colour)
    return case, Volume(vol['tsdf'], vol['weight'], vol['colour'], case['voxel'], case['origin'])


def plane_case(depth_value):
    """(a): one identity-pose camera (K of case_main's view 0) integrates a constant depth image into the 14 x 12 x 10 volume."""
    case = tsdf_ref.case_main()
    H, W = case['H'], case['W']
    K, pose = case['Ks'][:1], np.eye(4, dtype=np.float32)[None]
    depth = np.full((1, H, W), depth_value, np.float32)
    images = np.random.default_rng(11).uniform(0.0, 1.0, (1, 3, H, W)).astype(np.float32)
    vol = tsdf_ref.integrate(tsdf_ref.empty_volume(case['dims']), depth, images, K, pose, case['voxel'], case['origin'], case['trunc'], case['z_min'],
                             case['depth_max'])
    return dict(K=K, pose=pose, depth=depth, images=images, H=H, W=W, trunc=case['trunc'], voxel=case['voxel'], origin=case['origin'], dims=case['dims'],
                volume=Volume(vol['tsdf'], vol['weight'], vol['colour'], case['voxel'], case['origin']))


HOLE = (slice(4, 7), slice(4, 7), slice(5, 8))             # (iz, iy, ix): 3 x 3 x 3 nodes across the plane z = 1.7 of plane_case(1.7)


def holed_volume():
    """plane_case(1.7) with a 3 x 3 x 3 block of weight-0 nodes across the surface."""
    case = plane_case(1.7)
    v = case['volume']
    weight = v.weight.copy()
    weight[HOLE] = 0.0
    return case, Volume(v.tsdf, weight, v.colour, v.voxel, v.origin)


ODD = dict(nan=(4, 3, 3), inf=(6, 8, 9), light=(5, 6, 4))                           # (iz, iy, ix)
ZERO_PATCH = (5, slice(2, 6), slice(8, 12))                                          # 4 x 4 nodes of the layer iz = 5 set to an exact 0


def odd_volume():
    """plane_case(1.7) with a NaN node, a +inf node, a node of weight 0.5 (below min_weight = 1) and a patch of exact-0 nodes in the surface's
    cells: nodes of iz = 4 sit at z = 1.5625 (tsdf > 0), of iz = 5 at 1.6875 (> 0), of iz = 6 at 1.8125 (< 0).  A march that samples the
    planes of the nodes (z_start = 0.0625, step = 0.125) meets F = 0 exactly inside the patch."""
    case = plane_case(1.7)
    v = case['volume']
    tsdf, weight = v.tsdf.copy(), v.weight.copy()
    tsdf[ODD['nan']] = np.nan
    tsdf[ODD['inf']] = np.inf
    tsdf[ZERO_PATCH] = 0.0
    weight[ODD['light']] = 0.5
    return case, Volume(tsdf, weight, v.colour, v.voxel, v.origin)


ON_NODES = dict(z_start=0.0625, step=0.125, n_steps=25)    # every sample lies in a plane of nodes of the plane cases (f_z = 0)


def minimum_volume():
    """2 x 2 x 2 nodes, one cell: the field z-linear with its zero inside the cell, coloured; and a camera in front of it."""
    tsdf = np.empty((2, 2, 2), np.float32)
    tsdf[0], tsdf[1] = 0.75, -0.5
    tsdf[0, 1, 0] = 0.5
    colour = np.random.default_rng(2).uniform(0.0, 1.0, (2, 2, 2, 3)).astype(np.float32)
    vol = Volume(tsdf, np.ones((2, 2, 2), np.float32), colour, 0.25, (-0.25, -0.25, 1.0))
    K = np.array([[40.0, 0, 4.0], [0, 40.0, 5.0], [0, 0, 1]], np.float32)
    return vol, K, np.eye(4, dtype=np.float32)


def cameras():
    """Named cameras on case_main's volume (the box of node centres is [-0.8125, 0.8125] x [-0.6875, 0.6875] x [1.0625, 2.1875]):
    K, pose, and the march (z_start, step, n_steps)."""
    case = tsdf_ref.case_main()
    K0 = case['Ks'][0]
    wide = np.array([[24.0, 0, 15.5], [0, 24.0, 11.5], [0, 0, 1]], np.float32)
    out = dict(
        front=(K0, case['poses'][0], MAIN_STEPS),
        inside=(case['Ks'][1], case['poses'][1], MAIN_STEPS),
        away=(case['Ks'][2], case['poses'][2], MAIN_STEPS),
        # outside the box, oblique, a wide field of view: the border rays graze the box's edges and corners or miss it
        oblique=(wide, tsdf_ref.look_at((1.9, -1.4, 0.2), (0.1, 0.1, 1.7)), dict(z_start=0.0, step=0.125, n_steps=40)),
        # looking along +x from a point in the plane of the box's face y = -0.6875, cy an integer: the rays of row 12 run IN that face
        # (yr = 0, g_y = 0 exactly: valid), the rows above it outside the box, those below it inside
        grazing=(np.array([[30.0, 0, 15.5], [0, 31.0, 12.0], [0, 0, 1]], np.float32), tsdf_ref.look_at((-2.0, -0.6875, 1.6), (2.0, -0.6875, 1.6)),
                 dict(z_start=0.0, step=0.125, n_steps=40)),
        # far away: most k lie before the box
        far=(np.array([[120.0, 0, 15.5], [0, 120.0, 11.5], [0, 0, 1]], np.float32), tsdf_ref.look_at((0.2, 0.1, -6.0), (0.0, 0.0, 1.7)),
             dict(z_start=0.0, step=0.125, n_steps=80)),
        # from behind the surface
        behind=(K0, tsdf_ref.look_at((0.0, 0.0, 3.4), (0.0, 0.0, 1.7)), MAIN_STEPS))
    return out
