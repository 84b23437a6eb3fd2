"""The contract of ``sp_map_fuse`` (include/sp_hip.h) restated as an explicit loop over the points: float64 arithmetic on the float32
inputs, every operation rounded on its own (Python floats ARE IEEE float64 and round each + - * / once, exactly as NumPy's float64
does; the loop uses them because it visits every point), Python integers for the keys and the sums.  It also makes the cases of
tests/test_gpu_map_fuse.py and tests/test_map_fuse_ref_host.py.  Nothing here is a tolerance: the device result is compared bit for bit."""
import functools
import math

import numpy as np

HALF = 1 << 20                         # voxels to either side of the origin
SETTINGS = [(0.25, (0.0, 0.0, 0.0)), (0.3, (0.0, 0.0, 0.0)), (0.25, (0.1, -0.7, 3.3))]
BAD_ROWS = (11, 23, 31)                # of the random case: a NaN row, a row with +inf, a row at 1e7
NEG_ZERO_ROW = 5
FACE_EVERY = 97


def colour8(c):
    """The renderer's 8-bit value of a float32 colour channel: trunc of the exact float64 product, clamped; NaN gives 0."""
    p = float(c) * 255.0
    if not p > 0.0:
        return 0
    return 255 if p >= 255.0 else int(p)


def fuse(points, colours, voxel, origin):
    """points (Q,3) float32, colours (Q,3) float32 or None, voxel and origin as float32 values.  Returns dict(points (M,3) float32,
    colours (M,3) float32 or None, count (M,) int32, first (M,) int32, label (Q,) int32, n = M, and per fused row the exact quantities
    keys, sums (M,3) and colour_sums (M,3) as Python integers in object arrays)."""
    points = np.asarray(points, np.float32)
    Q = len(points)
    v = float(np.float32(voxel))
    o = [float(np.float32(x)) for x in origin]
    rows = points.astype(np.float64).tolist()              # float32 -> float64 is exact
    cols = None if colours is None else np.asarray(colours, np.float32).tolist()
    voxels = {}                                            # key -> [n, S, C, i0, g]; insertion order = ascending first row
    key_of = [None] * Q
    for i in range(Q):
        p = rows[i]
        q = [(p[a] - o[a]) / v for a in range(3)]
        if not all(math.isfinite(x) for x in q):
            continue
        g = [math.floor(x) for x in q]                     # exact integers
        if not all(-HALF <= x <= HALF - 1 for x in g):
            continue
        key = (g[0] + HALF) << 42 | (g[1] + HALF) << 21 | (g[2] + HALF)
        s = [min(int((q[a] - float(g[a])) * 65536.0), 65535) for a in range(3)]
        c8 = [0, 0, 0] if cols is None else [colour8(x) for x in cols[i]]
        key_of[i] = key
        e = voxels.get(key)
        if e is None:
            voxels[key] = [1, s, c8, i, g]
        else:
            e[0] += 1
            e[1] = [e[1][a] + s[a] for a in range(3)]
            e[2] = [e[2][a] + c8[a] for a in range(3)]
    M = len(voxels)
    row_of = {key: j for j, key in enumerate(voxels)}
    out_p, out_c = np.zeros((M, 3), np.float64), np.zeros((M, 3), np.float64)
    count, first = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for j, (key, (n, S, C, i0, g)) in enumerate(voxels.items()):
        count[j], first[j] = n, i0
        for a in range(3):
            m = float(S[a]) / float(n)
            c = (m + 0.5) / 65536.0
            out_p[j, a] = (float(g[a]) + c) * v + o[a]
            out_c[j, a] = float(C[a]) / (255.0 * float(n))
    label = np.array([-1 if k is None else row_of[k] for k in key_of], np.int32)
    return dict(points=out_p.astype(np.float32), colours=None if colours is None else out_c.astype(np.float32), count=count, first=first,
                label=label, n=M, keys=np.array(list(voxels), dtype=object),
                sums=np.array([e[1] for e in voxels.values()], dtype=object).reshape(M, 3),
                colour_sums=np.array([e[2] for e in voxels.values()], dtype=object).reshape(M, 3))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case_random(Q=5003, seed=501):
    """Coordinates uniform in +-2 (negative ones make floor differ from trunc); every 97th row rounded onto a face of the 0.25 grid
    through zero; row 5 is -0.0; the bad rows are a NaN row, a row with +inf and a row at 1e7 (out of range at every voxel size used);
    colours in -0.1 .. 1.1 with one NaN."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-2.0, 2.0, (Q, 3)).astype(np.float32)
    face = np.arange(0, Q, FACE_EVERY)
    p[face] = (np.round(p[face] / 0.25) * 0.25).astype(np.float32)
    if NEG_ZERO_ROW < Q:
        p[NEG_ZERO_ROW] = np.float32(-0.0)
    c = rng.uniform(-0.1, 1.1, (Q, 3)).astype(np.float32)
    if Q > max(BAD_ROWS):
        p[BAD_ROWS[0], 1] = np.nan
        p[BAD_ROWS[1], 2] = np.inf
        p[BAD_ROWS[2]] = np.float32(1e7)
        c[40, 1] = np.nan
    return p, c


@functools.lru_cache(maxsize=None)
def reference_random(setting, Q=5003, with_colours=True):
    p, c = case_random(Q)
    voxel, origin = SETTINGS[setting]
    return fuse(p, c if with_colours else None, voxel, origin)


@functools.lru_cache(maxsize=None)
def case_full_load(Q=4096, seed=502):
    """Q points, each alone in its voxel of side 0.5, in shuffled order: the table of 2 Q slots is exactly half full."""
    rng = np.random.default_rng(seed)
    cells = np.stack(np.unravel_index(rng.permutation(16 ** 3)[:Q], (16, 16, 16)), axis=1) - 8
    p = ((cells + rng.uniform(0.05, 0.95, (Q, 3))) * 0.5).astype(np.float32)
    c = rng.uniform(0.0, 1.0, (Q, 3)).astype(np.float32)
    return p, c, 0.5, (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def case_contention(n_voxels, Q=3000, seed=503):
    """Q points in ONE voxel of side 1 (n_voxels = 1), or alternating row by row between two voxels."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.001, 0.999, (Q, 3)).astype(np.float32)
    if n_voxels == 2:
        p[1::2, 2] -= np.float32(3.0)
    c = rng.uniform(0.0, 1.0, (Q, 3)).astype(np.float32)
    return p, c, 1.0, (0.0, 0.0, 0.0)
