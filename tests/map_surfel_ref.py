"""NumPy / Python float64 statements of the map normals and the surfel render (include/sp_hip.h: sp_map_normals, sp_render_surfels),
independent of the kernels and written as explicit loops: the normal of one table point with its neighbour search, the surfel render
with the winner of every pixel found by a loop over the points and their rectangles -- and the masks of tests/map_splat_ref.py,
generalised.  The projection, the half-widths and the rectangle are imported from map_render_ref / map_splat_ref, not restated.  The
inputs of every device case are made here too, so that the host tests can check them.

A Python float is an IEEE double and every Python operation on floats is rounded on its own: the loops below ARE the contract's
arithmetic (division by zero, which Python refuses, goes through ``_div``).

Masks (posed views only; with the identity pose there is no sum to reorder):
  position taint   map_splat_ref's, unchanged: a rectangle edge within DELTA px of an integer, or z within 1e-9 of z_min;
  t taint          a pixel some covering surfel gives a t within 1e-9 of z_min;
  cull taint       (cull = 1) every pixel of the rectangle of a surfel with |s| <= 1e-12 |n_c|_1 |p_c|_1: the sign of s is not safe;
  depth-tie taint  the two nearest covering t of a pixel agree within 5e-7 relative while neither their float32(t) nor their points
                   (coordinates, normal and radius) are identical."""
import math

import numpy as np

import map_render_ref as base
import map_splat_ref as splat
from map_render_ref import DELTA, TIE_RTOL, Z_MIN, camera, is_identity, pose_of  # noqa: F401  (the cases' tools)

INF = float("inf")
NAN = float("nan")


def _div(a, b):
    """IEEE a / b for Python floats (Python raises on b = 0)."""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return NAN
    return math.copysign(INF, a) * math.copysign(1.0, b)


# ---- sp_map_normals ----------------------------------------------------------------------------------------------------------------
def segment_of(seg_off, N, i):
    """The last segment whose offset is at or before table point i."""
    n = 0
    for k in range(N):
        if int(seg_off[k]) <= i:
            n = k
    return n


def neighbours(pix, lo, hi, i):
    """(left, right, up, down) of table point i inside its segment's range lo .. hi - 1, None where there is none.  Left and right
    must be the ADJACENT table points; up and down are searched for in the whole range (a plain scan: the kernel's binary search relies
    on the words being strictly increasing there)."""
    word = lambda k: int(pix[k]) & 0x7fffffff
    w = word(i)
    r, c = w >> 16, w & 0xffff
    left = i - 1 if i - 1 >= lo and c > 0 and word(i - 1) == (r << 16 | (c - 1)) else None
    right = i + 1 if i + 1 < hi and word(i + 1) == (r << 16 | (c + 1)) else None
    up = down = None
    for k in range(lo, hi):
        if r > 0 and word(k) == ((r - 1) << 16 | c):
            up = k
        if word(k) == ((r + 1) << 16 | c):
            down = k
    return left, right, up, down


class _Float64Of:
    """L(k) = float64(baseL[k])."""
    def __init__(self, values):
        self.values = values

    def __getitem__(self, k):
        return float(np.float32(self.values[k]))


def _difference(L, i, behind, ahead):
    if behind is not None and ahead is not None:
        return (L[ahead] - L[behind]) / 2.0
    if ahead is not None:
        return L[ahead] - L[i]
    if behind is not None:
        return L[i] - L[behind]
    return 0.0


def rotation(pose, rec=None):
    """R' as 3 x 3 Python floats: the pose's rotation, or rot_reanchor R with every entry as (a0 R0 + a1 R1) + a2 R2 in float64."""
    R = [[float(np.float32(pose[r][c])) for c in range(3)] for r in range(3)]
    if rec is None:
        return R
    A = [[float(rec['rot_reanchor'][r][c]) for c in range(3)] for r in range(3)]
    return [[(A[r][0] * R[0][c] + A[r][1] * R[1][c]) + A[r][2] * R[2][c] for c in range(3)] for r in range(3)]


def table_normal(tab, i, Rm):
    """The world normal (three Python floats, before the one rounding to float32) of table point i of ``tab`` = dict(pix, baseL,
    seg_off, N, P, K)."""
    pix, N, P = tab['pix'], int(tab['N']), int(tab['P'])
    n = segment_of(tab['seg_off'], N, i)
    lo = int(tab['seg_off'][n])
    hi = int(tab['seg_off'][n + 1]) if n + 1 < N else P
    L = _Float64Of(tab['baseL'])
    left, right, up, down = neighbours(pix, lo, hi, i)
    Lu, Lv = _difference(L, i, left, right), _difference(L, i, up, down)
    K = np.asarray(tab['K'], np.float32).reshape(3, 3)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    w = int(pix[i]) & 0x7fffffff
    r, c = float(w >> 16), float(w & 0xffff)
    m = (-(fx * Lu), -(fy * Lv), (1.0 + (c - cx) * Lu) + (r - cy) * Lv)
    if not all(math.isfinite(x) for x in m):
        return (0.0, 0.0, 0.0)
    length = math.sqrt((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2])
    nc = (_div(-m[0], length), _div(-m[1], length), _div(-m[2], length))
    return tuple((Rm[q][0] * nc[0] + Rm[q][1] * nc[1]) + Rm[q][2] * nc[2] for q in range(3))


def map_normals(tables, stride, poses, recs=None):
    """Every ``stride``-th table point of every table, keyframe after keyframe: (rows, 3) float64, to be rounded to float32 once."""
    out = []
    for k, tab in enumerate(tables):
        Rm = rotation(poses[k], None if recs is None else recs[k])
        tab = dict(tab, baseL=np.asarray(tab['baseL'], np.float32))
        for i in range(0, int(tab['P']), stride):
            out.append(table_normal(tab, i, Rm))
    return np.asarray(out, np.float64).reshape(-1, 3)


def table_from_masks(masks, L, K):
    """The table sp_table_fill builds from (N,H,W) masks and (N,H,W) log-depths: nonzero order, segment after segment."""
    N = masks.shape[0]
    pix, baseL, seg_off = [], [], []
    for n in range(N):
        seg_off.append(len(pix))
        for r, c in np.argwhere(masks[n]):
            pix.append(int(r) << 16 | int(c))
            baseL.append(L[n, r, c])
    seg_off.append(len(pix))
    return dict(pix=np.asarray(pix, np.uint32), baseL=np.asarray(baseL, np.float32), seg_off=np.asarray(seg_off, np.int32), N=N, P=len(pix),
                K=np.asarray(K, np.float32))


# ---- sp_render_surfels -------------------------------------------------------------------------------------------------------------
def usable(n):
    """The three floats are finite and not all zero."""
    return all(math.isfinite(float(x)) for x in n) and any(float(x) != 0.0 for x in n)


def view_normal(n, R):
    """n_c = R^T n, rows as (a + b) + c (n: three Python floats; R: 3 x 3 Python floats); R = None (the identity pose) leaves it untouched."""
    if R is None:
        return list(n)
    return [(R[0][q] * n[0] + R[1][q] * n[1]) + R[2][q] * n[2] for q in range(3)]


def _rotation_of(pose):
    if is_identity(pose):
        return None
    T = np.asarray(pose, np.float32).astype(np.float64)
    return [[float(T[r, c]) for c in range(3)] for r in range(3)]


def surfels(points, normals, radii, K, pose, H, W, max_px, z_min=Z_MIN):
    """Per kept (point, view), in ascending i: (i, rectangle, z, n_c or None for an unusable normal, s, h)."""
    u, v, z, ru, rv = splat.footprints(points, radii, K, pose, max_px)
    xs, ys, _ = base.camera_points(points, pose)
    keep = splat.kept(u, v, z, ru, rv, H, W, z_min)
    R = _rotation_of(pose)
    nl = np.asarray(normals, np.float32).astype(np.float64).tolist()
    rl = np.asarray(radii, np.float32).astype(np.float64).tolist()
    for i in np.nonzero(keep)[0].tolist():
        rect = splat.rectangle(u[i], v[i], ru[i], rv[i], H, W)
        zi = float(z[i])
        if not usable(nl[i]):
            yield i, rect, zi, None, 0.0, 0.0
            continue
        nc = view_normal(nl[i], R)
        s = (nc[0] * float(xs[i]) + nc[1] * float(ys[i])) + nc[2] * zi
        rad = rl[i]
        yield i, rect, zi, nc, s, 2.0 * (rad if rad >= 0.0 else 0.0)


def offers(points, normals, radii, K, pose, H, W, max_px, cull, z_min=Z_MIN):
    """Every (i, r, c, t, flat) a kept (point, view) makes on a pixel of its rectangle, in ascending i: t is the float64 depth BEFORE
    the test t > z_min and t < inf (``contested`` makes it); flat: the normal is unusable, the point's own z on every pixel.  A culled
    surfel yields nothing."""
    Kd = np.asarray(K, np.float32).astype(np.float64)
    fx, fy, cx, cy = float(Kd[0, 0]), float(Kd[1, 1]), float(Kd[0, 2]), float(Kd[1, 2])
    for i, (r0, r1, c0, c1), zi, nc, s, h in surfels(points, normals, radii, K, pose, H, W, max_px, z_min):
        if nc is None:
            for r in range(r0, r1 + 1):
                for c in range(c0, c1 + 1):
                    yield i, r, c, zi, True
            continue
        if cull and s >= 0.0:
            continue
        tl, th = zi - h, zi + h
        for r in range(r0, r1 + 1):
            b = ((r + 0.5) - cy) / fy
            for c in range(c0, c1 + 1):
                a = ((c + 0.5) - cx) / fx
                den = (nc[0] * a + nc[1] * b) + nc[2]
                t = _div(s, den)
                if t != t:
                    t = zi
                if t < tl:
                    t = tl
                if t > th:
                    t = th
                yield i, r, c, t, False


def contested(t, flat, z_min=Z_MIN):
    return flat or (t > float(np.float32(z_min)) and t < INF)


def render(points, colours, normals, radii, K, pose, H, W, max_px, cull=0, z_min=Z_MIN, made=None):
    """One view.  Returns image (H,W,3) uint8, depth (H,W) float32, index (H,W) int32: a point takes a pixel that is empty or whose
    holder's float32(t) is larger than or EQUAL to its own (it has the higher index).  ``made``: the list of ``offers`` of these very
    arguments, if the caller has it already."""
    index = np.full((H, W), -1, np.int32)
    best = np.zeros((H, W), np.float32)
    with np.errstate(over='ignore'):
        for i, r, c, t, flat in made if made is not None else offers(points, normals, radii, K, pose, H, W, max_px, cull, z_min):
            if not contested(t, flat, z_min):
                continue
            tf = np.float32(t)
            if index[r, c] < 0 or tf <= best[r, c]:
                index[r, c], best[r, c] = i, tf
    hit = index >= 0
    depth = np.where(hit, best, np.float32(0)).astype(np.float32)
    image = np.zeros((H, W, 3), np.uint8)
    if colours is not None:
        image[hit] = base.colour_u8(colours)[index[hit]]
    return image, depth, index


def t_taint(made, H, W, z_min=Z_MIN):
    """(H,W) bool from a list of ``offers``: some covering surfel gives the pixel a t within 1e-9 of z_min."""
    taint = np.zeros((H, W), bool)
    for i, r, c, t, flat in made:
        if not flat and abs(t - z_min) <= 1e-9:
            taint[r, c] = True
    return taint


def cull_taint(points, normals, radii, K, pose, H, W, max_px, z_min=Z_MIN):
    """cull = 1: the rectangle of every kept surfel whose |s| <= 1e-12 |n_c|_1 |p_c|_1."""
    xs, ys, zs = base.camera_points(points, pose)
    taint = np.zeros((H, W), bool)
    for i, (r0, r1, c0, c1), zi, nc, s, h in surfels(points, normals, radii, K, pose, H, W, max_px, z_min):
        if nc is not None and abs(s) <= 1e-12 * sum(abs(a) for a in nc) * (abs(float(xs[i])) + abs(float(ys[i])) + abs(zi)):
            taint[r0:r1 + 1, c0:c1 + 1] = True
    return taint


def depth_tie_taint(made, points, normals, radii, H, W, z_min=Z_MIN, rtol=TIE_RTOL):
    """(H,W) bool from a list of ``offers``: the two nearest contested t of the pixel agree within ``rtol`` relative while neither
    their float32(t) nor their points (coordinates, normal, radius) are identical."""
    first = np.full((H, W), -1, np.int64)
    second = np.full((H, W), -1, np.int64)
    t1 = np.full((H, W), np.inf)
    t2 = np.full((H, W), np.inf)
    for i, r, c, t, flat in made:
        if not contested(t, flat, z_min):
            continue
        if first[r, c] < 0 or t <= t1[r, c]:
            second[r, c], t2[r, c] = first[r, c], t1[r, c]
            first[r, c], t1[r, c] = i, t
        elif second[r, c] < 0 or t <= t2[r, c]:
            second[r, c], t2[r, c] = i, t
    row = np.concatenate([np.asarray(points, np.float32), np.asarray(normals, np.float32), np.asarray(radii, np.float32)[:, None]], axis=1)
    taint = np.zeros((H, W), bool)
    with np.errstate(over='ignore', invalid='ignore'):
        for r, c in zip(*np.nonzero(second >= 0)):
            a, b = t1[r, c], t2[r, c]
            close = abs(a - b) <= rtol * max(abs(a), abs(b))
            same_f32 = np.float32(a) == np.float32(b)
            same_point = np.array_equal(row[first[r, c]], row[second[r, c]], equal_nan=True)
            taint[r, c] = bool(close) and not same_f32 and not same_point
    return taint


def view_of(c, k, cull):
    """The statement's (image, depth, index) of view k of case ``c`` and the mask of the pixels to COMPARE: all of them for the identity
    pose, else those outside the four taints.  One walk over the offers serves both."""
    pose = None if 'poses' not in c else c['poses'][k]
    H, W = c['H'], c['W']
    made = list(offers(c['points'], c['normals'], c['radii'], c['K'], pose, H, W, c['max_px'], cull))
    want = render(c['points'], c['colours'], c['normals'], c['radii'], c['K'], pose, H, W, c['max_px'], cull, made=made)
    mask = np.ones((H, W), bool)
    if not is_identity(pose):
        taint = splat.position_taint(c['points'], c['radii'], c['K'], pose, H, W, c['max_px'])
        taint |= t_taint(made, H, W) | depth_tie_taint(made, c['points'], c['normals'], c['radii'], H, W)
        if cull:
            taint |= cull_taint(c['points'], c['normals'], c['radii'], c['K'], pose, H, W, c['max_px'])
        mask = ~taint
    return want, mask


# ---- the inputs of the device cases ------------------------------------------------------------------------------------------------
def unit_normals(n, seed):
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


def case_surfel_posed():
    """splat_posed (3001 points, three views of 30 x 40, max_px 3, half the cloud behind view 1) with random unit normals; every 11th
    normal is zero (a flat splat among surfels)."""
    c = dict(splat.case_splat_posed())
    normals = unit_normals(len(c['points']), 301)
    normals[::11] = 0.0
    c.update(normals=normals)
    return c


def case_surfel_views17():
    """splat_views17 (300 points, 17 views: one more than a staging chunk) with random unit normals."""
    c = dict(splat.case_splat_views17())
    c.update(normals=unit_normals(300, 302))
    return c


def case_surfel_collide():
    """splat_collide (70 001 points into 24 x 32, ids beyond 65 535, the identity pose and a posed view) with random unit normals."""
    c = dict(splat.case_splat_collide())
    c.update(normals=unit_normals(len(c['points']), 303))
    return c


EDGE_ROWS = dict(den_zero=0, grazing=1, zero_normal=2, nan_normal=3, inf_normal=4, s_zero=5, back=6, nan_radius=7, negative_radius=8,
                 zero_radius=9, inf_radius=10, huge_radius=11, near_plane=12, reaches=13, misses=14, corner=15)


def case_surfel_edges():
    """40 x 48, identity pose, K = (16, 16, 8, 8) -- so a = (c + 0.5 - 8) / 16 and b = (r + 0.5 - 8) / 16 are exact --, max_px 3,
    z_min 1e-6: sixteen constructed points (EDGE_ROWS names their rows).  No two rectangles overlap."""
    nan, inf = np.float32(np.nan), np.float32(np.inf)

    def at(u, v, z):
        return [(u - 8.0) * z / 16.0, (v - 8.0) * z / 16.0, z]
    rows = [
        # u = v = 4.5, z = 2, ru = 1: columns and rows 3..5.  n = (-1, 0, -0.28125), s = -0.125: at c = 3, a = -0.28125 and den = 0
        # exactly: t = -inf, clamped to z - h = 1.75; c = 4 gives t = z, c = 5 gives t = 1, clamped too
        (at(4.5, 4.5, 2.0), 0.125, [-1.0, 0.0, -0.28125]),
        # u = 12.9, v = 4.5, z = 2, radius 0.25 (ru = 2: columns 10..14), a grazing normal (-1, 0, 0.25), front-facing: t = 3.6 at
        # c = 12 (clamped to z + h = 2.5), 1.2 at c = 13 and negative at c = 11 (clamped to z - h = 1.5): both clamps are hit
        (at(12.9, 4.5, 2.0), 0.25, [-1.0, 0.0, 0.25]),
        (at(20.5, 4.5, 2.0), 0.125, [0.0, 0.0, 0.0]),            # zero normal: flat
        (at(28.5, 4.5, 2.0), 0.125, [nan, 0.5, 0.5]),            # NaN normal: flat
        (at(36.5, 4.5, 2.0), 0.125, [0.0, inf, -1.0]),           # infinite normal: flat
        # s = 0 exactly: p = (0.5, 0.25, 2), n = (2, 4, -1): 1 + 1 - 2 = 0.  cull = 1 drops it (s >= 0); cull = 0 gives t = 0 / den = 0,
        # clamped to z - h
        ([0.5, 0.25, 2.0], 0.125, [2.0, 4.0, -1.0]),
        (at(4.5, 20.5, 2.0), 0.125, [0.3, -0.2, 0.9]),           # back-facing (s > 0): drawn with cull = 0, dropped with cull = 1
        (at(12.5, 20.5, 2.0), nan, [0.3, 0.2, -0.9]),            # NaN radius: one pixel, h = 0, t = z
        (at(20.5, 20.5, 2.0), -0.5, [0.3, 0.2, -0.9]),           # negative radius: one pixel, t = z
        (at(28.5, 20.5, 2.0), 0.0, [0.3, 0.2, -0.9]),            # zero radius: one pixel, t = z
        (at(36.5, 20.5, 2.0), inf, [0.3, 0.2, -0.9]),            # infinite radius: the cap's 7 x 7, h = inf: no clamp
        (at(4.5, 30.5, 2.0), 1e9, [0.3, 0.2, -0.9]),             # radius 1e9: the cap's 7 x 7, no clamp in reach
        # z = 2e-6 > z_min with radius 1e-6 (h = 2e-6, ru = 8 -> cap 3): tilted so that some pixels have t <= z_min and are not drawn
        (at(14.5, 30.5, 2e-6), 1e-6, [0.9, 0.0, -0.4]),
        (at(-0.5, 36.5, 2.0), 0.125, [0.1, 0.1, -1.0]),          # u = -0.5, ru = 1: reaches column 0
        (at(-1.5, 30.5, 2.0), 0.125, [0.1, 0.1, -1.0]),          # u + ru = -0.5: misses
        (at(46.5, 38.5, 2.0), 1e9, [0.1, 0.1, -1.0]),            # the cap's square clipped to the corner: columns 43..47, rows 35..39
    ]
    pts = np.array([p for p, _, _ in rows], np.float32)
    radii = np.array([r for _, r, _ in rows], np.float32)
    normals = np.array([n for _, _, n in rows], np.float32)
    cols = np.linspace(0.05, 0.95, pts.size, dtype=np.float32).reshape(-1, 3)
    return dict(points=pts, colours=cols, normals=normals, K=camera(16.0, 16.0, 8.0, 8.0), H=40, W=48, radii=radii, max_px=3)


CASES = dict(surfel_posed=case_surfel_posed, surfel_views17=case_surfel_views17, surfel_collide=case_surfel_collide,
             surfel_edges=case_surfel_edges)
CULLS = dict(surfel_posed=(0, 1), surfel_views17=(0, 1), surfel_collide=(0,), surfel_edges=(0, 1))     # what the device test runs


# ---- the keyframes of the normals test ---------------------------------------------------------------------------------------------
LINEAR = dict(alpha=0.004, beta=-0.006, gamma=0.35)


def normal_scene():
    """Two keyframes as (masks (N,H,W) bool, L (N,H,W) float32, K (3,3) float32).
    A, 24 x 32, six segments: 0 the full image with L = alpha c + beta r + gamma (768 points: more than 256, so a row's up and down
    neighbours sit in another workgroup's rows); 1 one pixel; 2 one row; 3 a block with a hole; 4 and 5 two overlapping blocks with
    different L; segment 4 has a NaN in it.
    B, 17 x 21: one ragged segment (rows of differing extents)."""
    rng = np.random.default_rng(401)
    H, W = 24, 32
    A = np.zeros((6, H, W), bool)
    rr, cc = np.mgrid[0:H, 0:W]
    LA = (0.2 * rng.standard_normal((6, H, W)) + 0.6).astype(np.float32)
    A[0] = True
    LA[0] = (LINEAR['alpha'] * cc + LINEAR['beta'] * rr + LINEAR['gamma']).astype(np.float32)
    A[1, 7, 9] = True
    A[2, 11, 4:20] = True
    A[3, 3:9, 12:19] = True
    A[3, 5, 15] = False                                        # the hole
    A[4, 12:20, 5:15] = True
    A[5, 15:23, 10:22] = True                                  # overlaps segment 4 on rows 15..19, columns 10..14
    LA[4, 14, 8] = np.nan
    LA = np.where(A, LA, np.float32(0)).astype(np.float32)
    KA = camera(28.5, 29.25, 15.6, 11.3)
    H, W = 17, 21
    B = np.zeros((1, H, W), bool)
    for r in range(2, 15):
        a = 3 + (r * 5) % 7
        B[0, r, a:a + 4 + (r * 3) % 9] = True
    LB = np.where(B, (0.25 * rng.standard_normal((1, H, W)) + 0.4).astype(np.float32), np.float32(0)).astype(np.float32)
    KB = camera(19.0, 18.5, 10.2, 8.7)
    return [(A, LA, KA), (B, LB, KB)]


def case_plane(footprint):
    """map_splat_ref.case_plane -- the depth image gt = 1.5 + 0.01 c + 0.015 r sampled at every second pixel, the input whose flat
    render is pinned at 0.025 / 0.035 -- with the exact normal of the lifted surface p(u, v) = d(u, v) ((u - cx) / fx, (v - cy) / fy, 1)
    at every sample: -(dp/du x dp/dv), normalised in float64.  K_mid's centre is K's + 0.5, so the ray through the centre of pixel
    (r, c) under K_mid is the ray of the integer coordinate (c, r) under K: the ground truth at pixel-centre rays is gt[r, c] itself.
    A depth LINEAR in the pixel coordinates is not a plane in space (a plane has linear INVERSE depth): along the tangent plane of a
    sample of depth d0 the depth at pixel offset D is d0 / (1 - g . D / d0), g = (0.01, 0.015), against the surface's d0 + g . D: the
    difference is (g . D)^2 / (d0 - g . D) -- ``curvature`` bounds it for |D| <= floor(footprint / 2 + 0.5) per axis, d0 >= 1.5."""
    c = dict(splat.case_plane(footprint))
    Kd = c['K'].astype(np.float64)
    fx, fy, cx, cy = Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]
    rr, cc = np.mgrid[0:c['H'], 0:c['W']].astype(np.float64)
    r, col = rr[::2, ::2].reshape(-1), cc[::2, ::2].reshape(-1)
    d = 1.5 + 0.01 * col + 0.015 * r
    du = np.stack([(d + (col - cx) * 0.01) / fx, (r - cy) * 0.01 / fy, 0.01 + 0 * d], axis=-1)
    dv = np.stack([(col - cx) * 0.015 / fx, (d + (r - cy) * 0.015) / fy, 0.015 + 0 * d], axis=-1)
    n = -np.cross(du, dv)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    reach = np.floor(footprint / 2 + 0.5) * 0.025
    c.update(normals=n.astype(np.float32), curvature=reach ** 2 / (1.5 - reach))
    return c


TRUE_PLANE = dict(A=0.2, B=0.3, z0=1.8)


def case_true_plane(footprint):
    """A plane in SPACE, z = z0 + A x + B y, seen as map_splat_ref.case_plane sees its surface: 48 x 64, the same cameras, a sample at
    every second pixel in both directions lifted at its integer coordinate (float64, rounded to float32), radius footprint d / (2 fx),
    the plane's one unit normal (A, B, -1) / |.| on every point (it faces the camera: n . p = -z0 / |.| < 0).  Along the ray
    (X, Y, 1) the plane lies at z0 / (1 - A X - B Y); ``gt`` is that at the integer coordinates of K = the pixel centres of K_mid."""
    c = dict(splat.case_plane(footprint))
    A, B, z0 = TRUE_PLANE['A'], TRUE_PLANE['B'], TRUE_PLANE['z0']
    Kd = c['K'].astype(np.float64)
    fx, fy, cx, cy = Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]
    rr, cc = np.mgrid[0:c['H'], 0:c['W']].astype(np.float64)
    X, Y = (cc - cx) / fx, (rr - cy) / fy
    gt = z0 / (1.0 - A * X - B * Y)
    r, col = np.mgrid[0:c['H']:2, 0:c['W']:2]
    r, col = r.reshape(-1), col.reshape(-1)
    d = gt[r, col]
    pts = np.stack([X[r, col] * d, Y[r, col] * d, d], axis=1)
    n = np.array([A, B, -1.0]) / np.sqrt(A * A + B * B + 1.0)
    c.update(points=pts.astype(np.float32), radii=(footprint * d / (2.0 * fx)).astype(np.float32), gt=gt.astype(np.float32), gt64=gt,
             normals=np.tile(n, (len(d), 1)).astype(np.float32), normal64=n, rays=np.stack([X, Y, np.ones_like(X)], axis=-1))
    del c['bound']
    return c
