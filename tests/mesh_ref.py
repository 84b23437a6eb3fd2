"""NumPy / plain Python restatement of the mesh surfaces' rule (include/sp_hip.h: sp_mesh_faces, sp_mesh_sample), written from the header
and not from the kernel: float64 with every operation rounded on its own (NumPy and Python never contract), one rounding to float32 at
the end, ``mix`` on Python integers, and a plain loop over faces and samples for the order.  Test infrastructure only.  Also the meshes
the tests use (``sphere``, ``mixed``, ``skewed``, ``single``, ``strip``)."""
import math

import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
ONE = 1 << 53


def mix(x):
    """splitmix64's finaliser on a Python integer, modulo 2^64."""
    x &= MASK
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & MASK
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & MASK
    return x ^ (x >> 31)


def A(x):
    return mix(x) >> 11


def U(x):
    return float(A(x)) * 2.0 ** -53


def face_hash(seed, i):
    return (seed + GOLDEN * (i + 1)) & MASK


def face_records(vertices, faces):
    """vertices (M,3) float32, faces (F,3) int32.  Returns dict(area (F,) float64, normals (F,3) float32, state (F,) uint8, cross (F,3)
    float64, counts (5,) int64, area_max float)."""
    assert vertices.dtype == np.float32 and faces.dtype == np.int32 and vertices.ndim == 2 and faces.ndim == 2
    M, F = len(vertices), len(faces)
    state = np.zeros(F, np.uint8)
    area, cross, normals = np.zeros(F, np.float64), np.zeros((F, 3), np.float64), np.zeros((F, 3), np.float32)
    for i in range(F):
        idx = [int(k) for k in faces[i]]
        if any(k < 0 or k >= M for k in idx):
            state[i] = 1
            continue
        if idx[0] == idx[1] or idx[1] == idx[2] or idx[0] == idx[2]:
            state[i] = 2
            continue
        p = [[float(vertices[k, ax]) for ax in range(3)] for k in idx]
        if not all(math.isfinite(x) for row in p for x in row):
            state[i] = 3
            continue
        e1 = [p[1][ax] - p[0][ax] for ax in range(3)]
        e2 = [p[2][ax] - p[0][ax] for ax in range(3)]
        c = [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]
        length = math.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        a = 0.5 * length
        if not (a > 0.0 and math.isfinite(a)):
            state[i] = 4
            continue
        area[i], cross[i] = a, c
        normals[i] = [np.float32(c[ax] / length) for ax in range(3)]
    return dict(area=area, normals=normals, state=state, cross=cross, counts=np.bincount(state, minlength=5).astype(np.int64),
                area_max=float(area.max()) if F else 0.0)


def row_counts(vertices, faces, records, density, seed):
    """n_i of every face, Python integers."""
    M = len(vertices)
    out = []
    for i in range(len(faces)):
        if records['state'][i] != 0 or any(int(k) < 0 or int(k) >= M for k in faces[i]):
            out.append(0)
            continue
        t = float(records['area'][i]) * float(density)
        if not t < 2.0 ** 31:
            t = 2.0 ** 31
        out.append(max(0, int(math.floor(t + U(face_hash(seed, i))))))
    return out


def barycentric(seed, i, k):
    """(u1, u2) of row k of face i."""
    h = face_hash(seed, i)
    a1, a2 = A(h + 1 + 2 * k), A(h + 2 + 2 * k)
    if a1 + a2 > ONE:
        a1, a2 = ONE - a1, ONE - a2
    return float(a1) * 2.0 ** -53, float(a2) * 2.0 ** -53


def _blend(v, idx, u1, u2):
    p0, p1, p2 = (np.asarray(v[k], np.float64) for k in idx)
    return np.array([(float(p0[ax]) + u1 * (float(p1[ax]) - float(p0[ax]))) + u2 * (float(p2[ax]) - float(p0[ax])) for ax in range(3)]).astype(np.float32)


def sample(vertices, faces, records, density, seed, colours=None):
    """The cloud: dict(points, normals, colours (or None) (N,3) float32, face (N,) int32, n (F,) int64, u (N,2) float64, total)."""
    n = row_counts(vertices, faces, records, density, seed)
    total = sum(n)
    assert total < 5_000_000, "this loop is for test sizes"
    points, normals, face, u = np.zeros((total, 3), np.float32), np.zeros((total, 3), np.float32), np.zeros(total, np.int32), np.zeros((total, 2))
    cols = None if colours is None else np.zeros((total, 3), np.float32)
    row = 0
    for i, n_i in enumerate(n):
        idx = [int(k) for k in faces[i]]
        for k in range(n_i):
            u1, u2 = barycentric(seed, i, k)
            points[row] = _blend(vertices, idx, u1, u2)
            if cols is not None:
                cols[row] = _blend(colours, idx, u1, u2)
            normals[row] = records['normals'][i]
            face[row] = i
            u[row] = (u1, u2)
            row += 1
    return dict(points=points, normals=normals, colours=cols, face=face, n=np.array(n, np.int64), u=u, total=total)


def vertex_normals(vertices, faces, records):
    """``mesh_normals``' rule: per valid face q = round(c * (2^30 / c_max)) per component (float64, ties to even) as integers, c_max =
    2 area_max; the exact integer sum per vertex over its corners; normalised in float64, rounded to float32 once; a zero sum stays 0."""
    M = len(vertices)
    S = [[0, 0, 0] for _ in range(M)]
    c_max = 2.0 * records['area_max']
    scale = 2.0 ** 30 / c_max if c_max > 0 else 0.0
    for i in range(len(faces)):
        if records['state'][i] != 0:
            continue
        q = [int(np.rint(records['cross'][i, ax] * scale)) for ax in range(3)]
        for k in faces[i]:
            for ax in range(3):
                S[int(k)][ax] += q[ax]
    out = np.zeros((M, 3), np.float32)
    for m in range(M):
        s = [float(x) for x in S[m]]
        length = math.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
        if length > 0:
            out[m] = [np.float32(x / length) for x in s]
    return out


# ---- the meshes -----------------------------------------------------------------------------------------------------------------------------
def sphere():
    """The sphere of tests/tsdf_mesh_ref.py: 600 vertices, 1196 faces, colours."""
    import tsdf_mesh_ref as mref
    vol, mesh = mref.reference('sphere')
    return dict(vertices=mesh['vertices'], faces=mesh['faces'], colours=mesh['colours'], centre=vol['centre'], radius=vol['radius'])


def mixed():
    """Seven faces holding every state, bad faces between good ones: states 0, 1, 3, 0, 2, 4, 3 -- an index of -1 and one of M, a NaN and
    an inf coordinate, a repeated index, three collinear vertices.  Vertex 9 is referenced by no face."""
    v = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.25], [0.0, 2.0, 0.5], [1.0, 1.0, 3.0], [np.nan, 0.0, 1.0], [0.5, np.inf, 0.0],
                  [2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [4.0, 4.0, 4.0], [7.0, 7.0, 7.0]], np.float32)
    f = np.array([[0, 1, 2], [0, -1, 10], [0, 4, 1], [1, 3, 2], [2, 3, 2], [6, 7, 8], [3, 2, 5]], np.int32)
    c = np.linspace(0.0, 1.0, 30, dtype=np.float32).reshape(10, 3)
    return dict(vertices=v, faces=f, colours=c, states=[0, 1, 3, 0, 2, 4, 3])


def skewed(F=300, seed=5):
    """F faces: face 137 is one large triangle (area 60), the others are tiny (areas around 0.002): at density 20 the large one takes about
    1200 rows -- rows crossing several 256-row blocks --, most of the small ones take none, and the faces span two 256-face blocks."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(-1.0, 1.0, (F, 3))
    tri = base[:, None, :] + rng.uniform(-0.05, 0.05, (F, 3, 3))
    tri[137] = [[0.0, 0.0, 0.0], [12.0, 0.0, 1.0], [0.0, 10.0, -1.0]]
    v = tri.reshape(-1, 3).astype(np.float32)
    f = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    return dict(vertices=v, faces=f, colours=rng.uniform(0.0, 1.0, (3 * F, 3)).astype(np.float32))


def single():
    """F = 1."""
    v = np.array([[0.25, -1.0, 2.0], [1.75, 0.5, 2.5], [-0.5, 1.0, 3.0]], np.float32)
    return dict(vertices=v, faces=np.array([[0, 1, 2]], np.int32), colours=np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32))


def strip(F=257):
    """F faces of a triangle strip over F + 2 vertices on a wavy band: a second, partial 256-face block."""
    k = np.arange(F + 2, dtype=np.float64)
    v = np.stack([0.1 * k, (k % 2) + 0.05 * np.sin(k), 0.02 * k * np.cos(0.3 * k)], axis=1).astype(np.float32)
    f = np.stack([np.arange(F), np.arange(F) + 1, np.arange(F) + 2], axis=1).astype(np.int32)
    f[1::2] = f[1::2, ::-1]
    return dict(vertices=v, faces=np.ascontiguousarray(f), colours=None)


_cache = {}


def records_of(name):
    """(mesh, face records) of one of the meshes above, computed once; the tests leave both unchanged."""
    if name not in _cache:
        mesh = dict(sphere=sphere, mixed=mixed, skewed=skewed, single=single, strip=strip)[name]()
        _cache[name] = (mesh, face_records(mesh['vertices'], mesh['faces']))
    return _cache[name]


def sampled(name, density, seed):
    key = (name, float(density), int(seed))
    if key not in _cache:
        mesh, rec = records_of(name)
        _cache[key] = sample(mesh['vertices'], mesh['faces'], rec, density, seed, colours=mesh['colours'])
    return _cache[key]
