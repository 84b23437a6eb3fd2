"""NumPy restatement of the mesh views' rule (include/sp_hip.h: sp_mesh_render), written from the header and not from the kernel: float64
with every operation rounded on its own (NumPy and Python never contract), a plain loop over views and faces, the rule's test on the
rule's rectangle, the nearest-then-highest-index contest, one rounding to float32 at the end.  Test infrastructure only.  The meshes of
tests/mesh_ref.py are reused by import (``sphere``, ``mixed``, ``skewed``, ``single``, ``strip``); four more are made here: a two-triangle
slanted quad, a floor triangle that crosses the camera plane, one triangle larger than the image, and a duplicated face."""
import math

import numpy as np

from mesh_ref import mixed, records_of, single, skewed, sphere, strip  # noqa: F401  (the tests take them from here)

Z_MIN = 1e-6
H, W = 24, 32
INF = float("inf")


def camera(fx=20.0, fy=None, cx=15.5, cy=11.5):
    return np.array([[fx, 0, cx], [0, fx if fy is None else fy, cy], [0, 0, 1]], np.float32)


def identity():
    return np.eye(4, dtype=np.float32)


def pose(rotvec=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    """Camera-to-world, float32: Rodrigues' rotation of ``rotvec`` and the centre ``t``."""
    r = np.asarray(rotvec, np.float64)
    angle = float(np.linalg.norm(r))
    T = np.eye(4)
    if angle > 0:
        k = r / angle
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        T[:3, :3] = np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)
    T[:3, 3] = t
    return T.astype(np.float32)


def camera_point(T, p):
    """q = R^T (p - t), every row as (a + b) + c; an exact identity pose leaves the point untouched.  T float32 (4,4), p three floats."""
    R = [[float(T[r, c]) for c in range(3)] for r in range(3)]
    t = [float(T[r, 3]) for r in range(3)]
    if all(R[r][c] == (1.0 if r == c else 0.0) for r in range(3) for c in range(3)) and t == [0.0, 0.0, 0.0]:
        return [float(p[0]), float(p[1]), float(p[2])]
    d = [float(p[k]) - t[k] for k in range(3)]
    return [(R[0][r] * d[0] + R[1][r] * d[1]) + R[2][r] * d[2] for r in range(3)]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def pixel_of(K, q):
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    with np.errstate(all='ignore'):
        return float(np.float64(q[0] * fx) / np.float64(q[2]) + cx), float(np.float64(q[1] * fy) / np.float64(q[2]) + cy)


def usable(vertices, face):
    M = len(vertices)
    idx = [int(k) for k in face]
    if any(k < 0 or k >= M for k in idx) or idx[0] == idx[1] or idx[1] == idx[2] or idx[0] == idx[2]:
        return None
    if not all(math.isfinite(float(vertices[k, ax])) for k in idx for ax in range(3)):
        return None
    return idx


def face_setup(vertices, face, K, T, h, w, z_min, cull):
    """None for a face that covers nothing in this view, else dict(n (three edge planes), det, rect (c0, c1, r0, r1), whole)."""
    idx = usable(vertices, face)
    if idx is None:
        return None
    q = [camera_point(T, vertices[k]) for k in idx]
    n = [cross(q[1], q[2]), cross(q[2], q[0]), cross(q[0], q[1])]
    det = (q[0][0] * n[0][0] + q[0][1] * n[0][1]) + q[0][2] * n[0][2]
    if det == 0.0 or not math.isfinite(det):
        return None
    if cull and not det < 0.0:
        return None
    front = [qk[2] > z_min for qk in q]
    if not any(front):
        return None
    rect, whole = (0, w - 1, 0, h - 1), True
    if all(front):
        uv = [pixel_of(K, qk) for qk in q]
        if all(math.isfinite(x) for pair in uv for x in pair):
            whole = False
            us, vs = [p[0] for p in uv], [p[1] for p in uv]
            c0, c1 = max(math.floor(min(us)), 0.0), min(math.ceil(max(us)), float(w) - 1.0)
            r0, r1 = max(math.floor(min(vs)), 0.0), min(math.ceil(max(vs)), float(h) - 1.0)
            if not (c0 <= c1 and r0 <= r1):
                return None
            rect = (int(c0), int(c1), int(r0), int(r1))
    return dict(n=n, det=det, rect=rect, whole=whole, q=q)


def pixel_terms(s, K):
    """E (3, rows, cols), S, z and the covered mask -- without the test on z_min -- over the rectangle of set-up ``s``."""
    fx, fy, cx, cy = (np.float64(K[0, 0]), np.float64(K[1, 1]), np.float64(K[0, 2]), np.float64(K[1, 2]))
    c0, c1, r0, r1 = s['rect']
    a = ((np.arange(c0, c1 + 1, dtype=np.float64) - cx) / fx)[None, :]
    b = ((np.arange(r0, r1 + 1, dtype=np.float64) - cy) / fy)[:, None]
    with np.errstate(all='ignore'):
        E = np.stack([(np.float64(n[0]) * a + np.float64(n[1]) * b) + np.float64(n[2]) for n in s['n']])
        S = (E[0] + E[1]) + E[2]
        z = np.float64(s['det']) / S
    inside = ((E <= 0).all(axis=0) & (S < 0)) if s['det'] < 0 else ((E >= 0).all(axis=0) & (S > 0))
    return E, S, z, inside


def colour_u8(c32):
    p = c32.astype(np.float64) * 255.0
    out = np.zeros(p.shape, np.uint8)
    ok = p > 0.0
    out[ok] = np.where(p[ok] >= 255.0, 255, np.minimum(p[ok], 255.0).astype(np.int64)).astype(np.uint8)
    return out


def render_view(vertices, faces, K, T, h, w, z_min=Z_MIN, cull=0, colours=None, face_normals=None):
    """One view.  Returns depth (h,w) float32, normals (h,w,3) float32 or None, image (h,w,3) uint8 or None, index (h,w) int32, counts."""
    z_min = float(np.float32(z_min))
    depth, index = np.zeros((h, w), np.float32), np.full((h, w), -1, np.int32)
    image = None if colours is None else np.zeros((h, w, 3), np.uint8)
    whole = 0
    for f in range(len(faces)):
        s = face_setup(vertices, faces[f], K, T, h, w, z_min, cull)
        if s is None:
            continue
        whole += int(s['whole'])
        c0, c1, r0, r1 = s['rect']
        E, S, z, inside = pixel_terms(s, K)
        with np.errstate(all='ignore'):
            covered = inside & (z > z_min) & (z < INF)
            z32 = z.astype(np.float32)
        d, i = depth[r0:r1 + 1, c0:c1 + 1], index[r0:r1 + 1, c0:c1 + 1]            # (views into the images)
        wins = covered & ((i < 0) | (z32 <= d))                                   # faces come in ascending order: equal z, higher index
        d[wins], i[wins] = z32[wins], f
        if image is not None and wins.any():
            idx = [int(k) for k in faces[f]]
            with np.errstate(all='ignore'):
                lam = [E[k] / S for k in range(3)]
                for ch in range(3):
                    c = (lam[0] * np.float64(colours[idx[0], ch]) + lam[1] * np.float64(colours[idx[1], ch])) + lam[2] * np.float64(colours[idx[2], ch])
                    image[r0:r1 + 1, c0:c1 + 1, ch][wins] = colour_u8(c.astype(np.float32))[wins]
    normals = None
    if face_normals is not None:
        normals = np.full((h, w, 3), np.nan, np.float32)
        normals[index >= 0] = face_normals[index[index >= 0]]
    counts = dict(hits=int((index >= 0).sum()), faces=int(len(np.unique(index[index >= 0]))), whole=whole)
    return depth, normals, image, index, counts


def render(vertices, faces, Ks, poses, h, w, z_min=Z_MIN, cull=0, colours=None, face_normals=None):
    """V views: dict(depth, normals, image, index, counts); normals / image are None without face_normals / colours."""
    views = [render_view(vertices, faces, K, T, h, w, z_min, cull, colours, face_normals) for K, T in zip(Ks, poses)]
    stack = lambda k: None if views[0][k] is None else np.stack([v[k] for v in views])
    return dict(depth=stack(0), normals=stack(1), image=stack(2), index=stack(3), counts=[v[4] for v in views])


_cache = {}


def rendered(name, mesh, Ks, poses, h=H, w=W, cull=0, z_min=Z_MIN):
    """``render`` of a named case with the mesh's colours and its face normals (tests/mesh_ref.py's records), computed once per name; the
    tests leave the result unchanged."""
    key = (name, h, w, cull, z_min)
    if key not in _cache:
        from mesh_ref import face_records
        rec = face_records(mesh['vertices'], mesh['faces'])
        _cache[key] = (render(mesh['vertices'], mesh['faces'], Ks, poses, h, w, z_min, cull, mesh.get('colours'), rec['normals']), rec)
    return _cache[key]


# ---- the meshes of this file ----------------------------------------------------------------------------------------------------------
def quad():
    """Two triangles sharing the diagonal 0-2 of a slanted quadrilateral on the plane z = 2 + 0.25 x + 0.5 y: every coordinate is exact in
    float32, so the four vertices are exactly coplanar."""
    xy = [(-1.0, -0.75), (1.25, -0.5), (1.0, 0.875), (-0.75, 0.5)]
    v = np.array([[x, y, 2.0 + 0.25 * x + 0.5 * y] for x, y in xy], np.float32)
    c = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0]], np.float32)
    return dict(vertices=v, faces=np.array([[0, 1, 2], [0, 2, 3]], np.int32), colours=c, plane=(0.25, 0.5, 2.0))


def floor(flipped=False):
    """One triangle of the plane y = 1 (below an identity camera: y points down) from z = -10 behind the camera to z = 60 in front."""
    v = np.array([[-100.0, 1.0, -10.0], [100.0, 1.0, -10.0], [0.0, 1.0, 60.0]], np.float32)
    f = [0, 2, 1] if flipped else [0, 1, 2]
    return dict(vertices=v, faces=np.array([f], np.int32), colours=np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32))


def oversized():
    """One triangle at depths 2 to 4 whose projection contains a 40 x 56 image many times over; all three vertices are in front."""
    v = np.array([[-60.0, -40.0, 2.0], [70.0, -35.0, 3.0], [0.0, 90.0, 4.0]], np.float32)
    return dict(vertices=v, faces=np.array([[0, 1, 2]], np.int32), colours=np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32))


def behind():
    """``single`` mirrored behind an identity camera."""
    m = single()
    v = m['vertices'].copy()
    v[:, 2] = -v[:, 2]
    return dict(vertices=v, faces=m['faces'], colours=m['colours'])


def duplicate():
    """``single``'s triangle twice, and a third, farther one that loses wherever the two lie."""
    m = single()
    v = np.concatenate([m['vertices'], m['vertices'] + np.array([0.6, 0, 1.5], np.float32)]).astype(np.float32)
    return dict(vertices=v, faces=np.array([[0, 1, 2], [0, 1, 2], [3, 4, 5]], np.int32), colours=np.concatenate([m['colours'], m['colours'][::-1]]))


def unusable():
    """No usable face: an index outside the vertices, a repeated index, a NaN coordinate."""
    v = np.array([[0.0, 0.0, 2.0], [1.0, 0.0, 2.0], [0.0, 1.0, 2.0], [np.nan, 0.0, 2.0]], np.float32)
    return dict(vertices=v, faces=np.array([[0, 1, 4], [0, 1, 1], [0, 3, 2], [-1, 1, 2]], np.int32), colours=np.ones((4, 3), np.float32))


def sphere_views():
    """The cameras of the sphere: from its centre, from 4 r in front of it, and a grazing one whose image border cuts the silhouette."""
    m = sphere()
    c, r = np.asarray(m['centre'], np.float64), float(m['radius'])
    return dict(centre=pose(t=c), outside=pose(t=c - np.array([0, 0, 4 * r])), grazing=pose(rotvec=(0.0, 0.42, 0.0), t=c - np.array([0.3 * r, 0.1 * r, 2.5 * r])))


def cases():
    """The cases the device is held to, name -> (mesh, Ks (V,3,3), poses (V,4,4), h, w): every mesh from a camera that sees what the
    case is about (tests/test_mesh_render_host.py asserts that it does)."""
    sv = sphere_views()
    one = lambda K, T: (np.stack([K]), np.stack([T]))
    out = {
        'sphere from its centre': (sphere(), *one(camera(6.0), sv['centre']), H, W),
        'sphere from outside': (sphere(), *one(camera(20.0), sv['outside']), H, W),
        'sphere grazing': (sphere(), *one(camera(20.0), sv['grazing']), 21, 30),
        'mixed': (mixed(), *one(camera(20.0), pose((0.0, -0.8, 0.0), (3.5, 0.8, -2.0))), H, W),
        'skewed': (skewed(), *one(camera(20.0), pose(t=(0.0, 0.0, -0.4))), 21, 30),
        'skewed from afar': (skewed(), *one(camera(10.0), pose(t=(1.0, 1.0, -4.0))), H, W),
        'strip': (strip(257), *one(camera(6.0, 40.0), pose((0.0, 0.1, 0.05), (13.0, 0.5, -4.0))), 21, 30),
        'single': (single(), *one(camera(20.0), identity()), H, W),
        'floor': (floor(), *one(camera(20.0), identity()), 21, 30),
        'oversized': (oversized(), *one(camera(20.0), identity()), 40, 56),
        'duplicate': (duplicate(), *one(camera(20.0), identity()), 21, 30),
        'quad': (quad(), *one(camera(20.0), pose((0.2, -0.3, 0.1), (0.3, -0.2, -1.0))), H, W),
        'unusable': (unusable(), *one(camera(20.0), identity()), H, W),
    }
    return out
