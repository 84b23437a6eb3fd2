"""The contracts of ``sp_cloud_grid_knn`` and ``sp_cloud_normals`` (include/sp_hip.h) restated in float64 NumPy on the float32 inputs.
The range test, the parameters and d2 are those of tests/map_nearest_ref.py (imported, not copied): the neighbours of a query are
exactly those of ``sp_cloud_grid_nearest``.

``knn``             all pairs: every query against every reference row, the neighbours sorted by ``np.lexsort`` on (row, d2).
``knn_candidates``  for the larger sizes, independent of the first: candidates from ``cKDTree.query_ball_point`` at 1.001 r (a superset),
                    decided and ranked among in the contract's arithmetic, vectorised over all pairs at once.
``normals``         the covariance built exactly as the contract writes it (sums in list order), then ``numpy.linalg.eigh`` -- another
                    backward-stable solver than the kernel's Jacobi sweeps: the comparison carries a gap-scaled bound (``angle_bound``).

The lists are compared bit for bit; nothing here is a tolerance but ``angle_bound`` and ``curvature_bound``."""
import functools

import numpy as np

from map_nearest_ref import _d2, cells, cloud, parameters

KNN_MAX = 32


def _empty(Qa, k):
    return dict(index=np.full((Qa, k), -1, np.int32), d2=np.full((Qa, k), np.inf), count=np.zeros(Qa, np.int32))


def _finish(out):
    out['dist'] = np.sqrt(out['d2']).astype(np.float32)
    return out


def _clouds(queries, points, radius, origin):
    r2, cell, o = parameters(radius, origin)
    a, b = np.asarray(queries, np.float32).astype(np.float64), np.asarray(points, np.float32).astype(np.float64)
    return r2, a, b, cells(queries, cell, o)[0], cells(points, cell, o)[0]


def knn(queries, points, radius, origin, k, skip_self=False):
    """All pairs.  Returns dict(index (Qa,k) int32, dist (Qa,k) float32, count (Qa,) int32, d2 (Qa,k) float64 -- -1 / inf padding)."""
    r2, a, b, ok_a, ok_b = _clouds(queries, points, radius, origin)
    out = _empty(len(a), k)
    rows = np.arange(len(b))
    for i in np.nonzero(ok_a)[0]:
        d2 = _d2(a[i], b)
        with np.errstate(invalid='ignore'):
            hit = ok_b & (d2 <= r2)
        if skip_self:
            hit[i] = False
        j = rows[hit]
        best = j[np.lexsort((j, d2[j]))[:k]]               # ascending (d2, j)
        out['index'][i, :len(best)], out['d2'][i, :len(best)], out['count'][i] = best, d2[best], len(j)
    return _finish(out)


def knn_candidates(queries, points, radius, origin, k, skip_self=False):
    """Candidates from a k-d tree over the in-range reference rows at 1.001 r, then the contract's arithmetic on all pairs at once."""
    from scipy.spatial import cKDTree
    r2, a, b, ok_a, ok_b = _clouds(queries, points, radius, origin)
    out = _empty(len(a), k)
    rows_a, rows_b = np.nonzero(ok_a)[0], np.nonzero(ok_b)[0]
    if not len(rows_a) or not len(rows_b):
        return _finish(out)
    found = cKDTree(b[rows_b]).query_ball_point(a[rows_a], float(np.float32(radius)) * 1.001, return_sorted=False)
    n = np.array([len(f) for f in found])
    if not n.sum():
        return _finish(out)
    qi = np.repeat(rows_a, n)
    j = rows_b[np.concatenate([np.asarray(f, np.int64) for f in found]).astype(np.int64)]
    d2 = _d2(a[qi], b[j])
    hit = d2 <= r2
    if skip_self:
        hit &= qi != j
    qi, j, d2 = qi[hit], j[hit], d2[hit]
    out['count'][:] = np.bincount(qi, minlength=len(a))
    order = np.lexsort((j, d2, qi))
    qi, j, d2 = qi[order], j[order], d2[order]
    start = np.concatenate([[0], np.cumsum(out['count'])])[qi]     # where the group of query qi begins in the sorted pairs
    rank = np.arange(len(qi)) - start
    top = rank < k
    out['index'][qi[top], rank[top]], out['d2'][qi[top], rank[top]] = j[top], d2[top]
    return _finish(out)


def same(got, want):
    """Exact: index and count equal, dist equal as bit patterns."""
    return (np.array_equal(got['index'], want['index']) and np.array_equal(got['count'], want['count'])
            and np.array_equal(np.asarray(got['dist'], np.float32).view(np.uint32), want['dist'].view(np.uint32)))


# ---- normals -------------------------------------------------------------------------------------------------------------------------
TINY_GAP = 2.0 ** -30


def normals(points, queries, index, toward=None, owner=None):
    """The contract of sp_cloud_normals with ``numpy.linalg.eigh`` as the solver.  Returns dict(normals (Qa,3) float64 -- NOT yet rounded
    to float32 --, curvature (Qa,) float64, used (Qa,) int32, gap (Qa,) float64 = l2 / (l1 - l0), evals (Qa,3))."""
    p32, index = np.asarray(points, np.float32), np.asarray(index, np.int64)
    p, q = p32.astype(np.float64), np.asarray(queries, np.float32).astype(np.float64)
    Q, (Qa, k) = len(p), index.shape
    S1, S2, used = np.zeros((Qa, 3)), np.zeros((Qa, 6)), np.zeros(Qa, np.int32)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    with np.errstate(invalid='ignore', over='ignore'):
        for n in range(k):                                 # list order; adding 0.0 for a skipped entry changes no sum
            r = index[:, n]
            inside = (r >= 0) & (r < Q)
            r = np.where(inside, r, 0)
            take = inside & np.isfinite(p32[r]).all(axis=1)
            d = np.where(take[:, None], p[r] - q, 0.0)
            S1 += d
            for c, (u, v) in enumerate(pairs):
                S2[:, c] += d[:, u] * d[:, v]
            used += take
        N = np.maximum(used, 1).astype(np.float64)[:, None]
        m = S1 / N
        cov = S2 / N - np.stack([m[:, u] * m[:, v] for u, v in pairs], axis=1)
    C = np.empty((Qa, 3, 3))
    for c, (u, v) in enumerate(pairs):
        C[:, u, v] = C[:, v, u] = cov[:, c]
    solvable = (used >= 3) & np.isfinite(C).all(axis=(1, 2))
    C[~solvable] = np.eye(3)
    evals, evecs = np.linalg.eigh(C)                       # ascending
    l0, l1, l2 = evals[:, 0], evals[:, 1], evals[:, 2]
    ok = solvable & (l1 > TINY_GAP * l2)
    e = evecs[:, :, 0].copy()
    e /= np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])[:, None]
    lead = np.argmax(np.abs(e), axis=1)                    # (the first of equal magnitudes: the lowest axis)
    flip = e[np.arange(Qa), lead] < 0
    if toward is not None:
        views = np.asarray(toward, np.float32).astype(np.float64).reshape(-1, 3)
        o = np.zeros(Qa, np.int64) if owner is None else np.asarray(owner, np.int64)
        has = (o >= 0) & (o < len(views))
        c = views[np.where(has, o, 0)] - q
        with np.errstate(invalid='ignore'):
            dot = (e[:, 0] * c[:, 0] + e[:, 1] * c[:, 1]) + e[:, 2] * c[:, 2]
            flip = np.where(has & (dot < 0), True, np.where(has & (dot > 0), False, flip))
    e[flip] = -e[flip]
    with np.errstate(invalid='ignore', divide='ignore'):
        curvature = np.maximum(l0, 0.0) / ((l0 + l1) + l2)
        gap = l2 / (l1 - l0)
    e[~ok], curvature[~ok], gap[~ok] = np.nan, np.nan, np.nan
    return dict(normals=e, curvature=curvature, used=used, gap=gap, evals=evals)


def angle(u, v):
    """The angle between the LINES through u and v, row by row (the sign of an eigenvector is tested apart): atan2(|u x v|, |u . v|)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(u, v), axis=1), np.abs((u * v).sum(axis=1)))


def angle_bound(gap):
    """2^-22 for the float32 rounding of three components, and a Davis-Kahan term with the constant 64 over float64's unit roundoff for
    two different backward-stable 3 x 3 solvers."""
    return 2.0 ** -22 + 64 * 2.0 ** -52 * gap


def curvature_bound(curvature):
    return 128 * 2.0 ** -52 + 2.0 ** -23 * curvature


# ---- the cases -------------------------------------------------------------------------------------------------------------------------
RANDOM_CASES = [(0, 3), (1, 3), (0, 8), (1, 8)]            # (setting of map_nearest_ref.SETTINGS, k)
SELF_RADIUS, SELF_K = 0.4, 8


@functools.lru_cache(maxsize=None)
def reference_random(setting, k):
    """map_nearest_ref.case_random() at one of its settings: all pairs, computed once."""
    import map_nearest_ref as base
    a, b = base.case_random()
    return knn(a, b, *base.SETTINGS[setting], k)


@functools.lru_cache(maxsize=None)
def reference_self():
    """The 3001 random reference points against themselves at r = 0.4 with skip_self, k = 8."""
    import map_nearest_ref as base
    b = base.case_random()[1]
    return knn(b, b, SELF_RADIUS, (0.0, 0.0, 0.0), SELF_K, skip_self=True)


@functools.lru_cache(maxsize=None)
def sphere(Q=4001, seed=7):
    """Q points on the unit sphere: normal deviates normalised in float64, cast to float32."""
    g = np.random.default_rng(seed).normal(size=(Q, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sphere_lists(radius, k):
    p = sphere()
    return knn_candidates(p, p, radius, (0.0, 0.0, 0.0), k)


def small_cloud(Q=600, seed=611):
    """A cloud of the random kind (a NaN row, a +inf row, a far row, a -0.0 row) dense enough for lists of 32 at r = 0.9."""
    return cloud(Q, seed)
