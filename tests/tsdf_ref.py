"""NumPy restatement of sp_tsdf_integrate's rule (include/sp_hip.h), written from the rule and not from the kernel: float64 geometry from
the float32 inputs, every operation on its own, and an update in np.float32 whose every operation is rounded on its own.  Test
infrastructure only.  Also the two volumes' worth of inputs the GPU test integrates (``case_main``, ``case_small``)."""
import numpy as np


def node_centres(n, voxel, o):
    """p_a = ((float64(i_a) + 0.5) * voxel) + o_a for i_a = 0 .. n-1."""
    return ((np.arange(n, dtype=np.float64) + 0.5) * np.float64(np.float32(voxel))) + np.float64(np.float32(o))


def empty_volume(dims, colour=True):
    nx, ny, nz = dims
    return dict(tsdf=np.zeros((nz, ny, nx), np.float32), weight=np.zeros((nz, ny, nx), np.float32),
                colour=np.zeros((nz, ny, nx, 3), np.float32) if colour else None)


def integrate(vol, depth, images, Ks, poses, voxel, origin, trunc, z_min, depth_max, stats=None):
    """``vol`` (what ``empty_volume`` made) is updated in place by the V views in order.  depth (V,H,W) float32, images (V,3,H,W) float32
    or None, Ks (V,3,3) float32, poses (V,4,4) float32 camera-to-world.  ``stats``: a list that gets one dict of counts per view."""
    tsdf, weight, colour = vol['tsdf'], vol['weight'], vol['colour']
    nz, ny, nx = tsdf.shape
    V, H, W = depth.shape
    assert depth.dtype == np.float32 and Ks.dtype == np.float32 and poses.dtype == np.float32 and (images is None) == (colour is None)
    px = node_centres(nx, voxel, origin[0])[None, None, :]
    py = node_centres(ny, voxel, origin[1])[None, :, None]
    pz = node_centres(nz, voxel, origin[2])[:, None, None]
    tr, zmin, dmax = np.float64(np.float32(trunc)), np.float64(np.float32(z_min)), np.float32(depth_max)
    one = np.float32(1.0)
    for v in range(V):
        T, K = poses[v].astype(np.float64), Ks[v].astype(np.float64)
        d0, d1, d2 = px - T[0, 3], py - T[1, 3], pz - T[2, 3]
        # p_c = R^T d: row r of R^T is column r of R; three-term sums as (a + b) + c
        x = (T[0, 0] * d0 + T[1, 0] * d1) + T[2, 0] * d2
        y = (T[0, 1] * d0 + T[1, 1] * d1) + T[2, 1] * d2
        z = (T[0, 2] * d0 + T[1, 2] * d1) + T[2, 2] * d2
        x, y, z = np.broadcast_to(x, tsdf.shape), np.broadcast_to(y, tsdf.shape), np.broadcast_to(z, tsdf.shape)
        front = z > zmin
        with np.errstate(all='ignore'):
            u = (x * K[0, 0]) / z + K[0, 2]
            w = (y * K[1, 1]) / z + K[1, 2]
            col, row = np.floor(u + 0.5), np.floor(w + 0.5)
        inside = front & np.isfinite(col) & np.isfinite(row) & (col >= 0) & (col < W) & (row >= 0) & (row < H)
        c = np.where(inside, col, 0).astype(np.int64)
        r = np.where(inside, row, 0).astype(np.int64)
        D = depth[v][r, c]
        with np.errstate(all='ignore'):
            good = inside & np.isfinite(D) & (D > 0) & (D <= dmax)
            sdf = D.astype(np.float64) - z
            kept = good & ~(sdf < -tr)
            s = np.minimum(1.0, sdf / tr).astype(np.float32)
            wn = weight + one                                                          # float32, each operation rounded on its own
            new_tsdf = (tsdf * weight + s) / wn
            if colour is not None:
                e = images[v][:, r, c]                                                 # (3, nz, ny, nx)
                e = np.where(np.isnan(e), np.float32(0), e)
                new_colour = (colour * weight[..., None] + np.moveaxis(e, 0, -1)) / wn[..., None]
        assert new_tsdf.dtype == np.float32 and wn.dtype == np.float32
        if colour is not None:
            assert new_colour.dtype == np.float32
            colour[...] = np.where(kept[..., None], new_colour, colour)
        tsdf[...] = np.where(kept, new_tsdf, tsdf)
        weight[...] = np.where(kept, wn, weight)
        if stats is not None:
            with np.errstate(all='ignore'):
                stats.append(dict(behind=int((~front).sum()), outside=int((front & ~inside).sum()), bad_depth=int((inside & ~good).sum()),
                                  nan=int((inside & np.isnan(D)).sum()), zero=int((inside & (D == 0)).sum()), negative=int((inside & (D < 0)).sum()),
                                  inf=int((inside & np.isposinf(D)).sum()), beyond=int((inside & np.isfinite(D) & (D > dmax)).sum()),
                                  hidden=int((good & ~kept).sum()), updated=int(kept.sum()), clipped=int((kept & (sdf >= tr)).sum()),
                                  at_minus_trunc=int((kept & (sdf == -tr)).sum()), at_trunc=int((kept & (sdf == tr)).sum())))
    return vol


def look_at(eye, target, up=(0.0, -1.0, 0.0)):
    """A camera-to-world pose (float32) at ``eye`` whose +z axis points at ``target`` (x right, y down)."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    zc = target - eye
    zc /= np.linalg.norm(zc)
    xc = np.cross(-np.asarray(up, np.float64), zc)
    xc /= np.linalg.norm(xc)
    yc = np.cross(zc, xc)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2], T[:3, 3] = xc, yc, zc, eye
    return T.astype(np.float32)


def plane_depth(K, T, H, W, normal, offset):
    """The depth image (float32) a camera sees of the plane normal . p = offset (0 where the ray misses it or meets it behind the camera)."""
    K, T = K.astype(np.float64), T.astype(np.float64)
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    rays = np.stack([(c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1], np.ones_like(c)], axis=-1)      # camera frame, z = 1
    n_c = T[:3, :3].T @ np.asarray(normal, np.float64)
    denom = rays @ n_c
    with np.errstate(all='ignore'):
        d = (offset - np.asarray(normal, np.float64) @ T[:3, 3]) / denom
    return np.where(np.isfinite(d) & (d > 0), d, 0.0).astype(np.float32)


MAIN = dict(dims=(14, 12, 10), voxel=0.125, origin=(-0.875, -0.75, 1.0), trunc=0.5, z_min=1e-6, depth_max=3.0, H=24, W=32)


def case_main():
    """14 x 12 x 10 nodes of side 1/8 (every node centre is a dyadic number: z in camera 0, which only translates, is exact), three views
    of 24 x 32 with their own Ks: view 0 in front of the volume looking down +z, view 1 INSIDE the volume and turned (part of the volume
    is behind it), view 2 looking away (it sees none of it).  The depth images show the slanted plane 0.25 x + 0.125 y + z = 1.75; into
    them are seeded NaN, 0, a negative value, +inf, a value beyond depth_max, and -- in view 0 -- two pixels whose depth puts one node
    exactly at sdf = -trunc and one exactly at sdf = +trunc."""
    c = dict(MAIN)
    H, W = c['H'], c['W']
    Ks = np.array([[[30.0, 0, 15.5], [0, 31.0, 11.5], [0, 0, 1]], [[22.0, 0, 16.25], [0, 21.0, 12.0], [0, 0, 1]],
                   [[28.0, 0, 15.0], [0, 28.0, 12.5], [0, 0, 1]]], np.float32)
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = (0.0625, -0.03125, 0.25)
    T1 = look_at((0.3, -0.2, 1.55), (-0.35, 0.3, 2.2))
    T2 = look_at((0.0, 0.0, 0.5), (0.1, 0.2, -1.0))
    poses = np.stack([T0, T1, T2])
    normal, offset = (0.25, 0.125, 1.0), 1.75
    depth = np.stack([plane_depth(Ks[v], poses[v], H, W, normal, offset) for v in range(3)])
    rng = np.random.default_rng(5)
    images = rng.uniform(0.0, 1.0, (3, 3, H, W)).astype(np.float32)
    images[0, 1, 10:13, 14:18] = np.nan                                                # a NaN colour is taken as 0
    for v in (0, 1):                                                                   # the five kinds of depth that are no surface
        depth[v, 5, 12:15] = np.nan
        depth[v, 8, 16:19] = 0.0
        depth[v, 11, 9:12] = -1.5
        depth[v, 14, 18:21] = np.inf
        depth[v, 17, 13:16] = 3.5                                                      # > depth_max = 3
    # view 0 only translates: z = p_z - t_z exactly.  Node (6, 5, 4) gets sdf = -trunc, node (9, 7, 2) sdf = +trunc (no other node of
    # their pixels' rays matters to the claim: the statistics of the reference are what the test asserts)
    for (ix, iy, iz), sign in (((6, 5, 4), -1.0), ((9, 7, 2), 1.0)):
        p = [node_centres(n, c['voxel'], o)[i] for n, o, i in zip(c['dims'], c['origin'], (ix, iy, iz))]
        x, y, z = p[0] - float(T0[0, 3]), p[1] - float(T0[1, 3]), p[2] - float(T0[2, 3])
        col, row = int(np.floor(x * 30.0 / z + 15.5 + 0.5)), int(np.floor(y * 31.0 / z + 11.5 + 0.5))
        value = np.float32(z + sign * c['trunc'])
        assert float(value) == z + sign * c['trunc'] and 0 <= col < W and 0 <= row < H
        depth[0, row, col] = value
    c.update(Ks=Ks, poses=poses, depth=depth, images=images)
    return c


def case_small():
    """5 x 3 x 2 nodes and one view: partial waves, one partial block."""
    H, W = 9, 11
    K = np.array([[[12.0, 0, 5.0], [0, 12.0, 4.0], [0, 0, 1]]], np.float32)
    pose = look_at((0.05, -0.1, -0.6), (0.3, 0.2, 0.2))[None]
    depth = plane_depth(K[0], pose[0], H, W, (0.1, -0.2, 1.0), 0.15)[None]
    images = np.random.default_rng(6).uniform(0.0, 1.0, (1, 3, H, W)).astype(np.float32)
    return dict(dims=(5, 3, 2), voxel=0.1, origin=(0.0, 0.0, 0.0), trunc=0.3, z_min=1e-6, depth_max=10.0, H=H, W=W, Ks=K, poses=pose, depth=depth,
                images=images)


def reference(case, views=None, vol=None, colour=True, stats=None):
    """The case's views (a slice, default all) integrated into ``vol`` (default: a fresh volume)."""
    vol = empty_volume(case['dims'], colour) if vol is None else vol
    sl = slice(None) if views is None else views
    return integrate(vol, case['depth'][sl], case['images'][sl] if colour else None, case['Ks'][sl], case['poses'][sl], case['voxel'], case['origin'],
                     case['trunc'], case['z_min'], case['depth_max'], stats=stats)
