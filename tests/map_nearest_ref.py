"""The contract of ``sp_cloud_grid_build`` / ``sp_cloud_grid_nearest`` (include/sp_hip.h) restated in float64 NumPy on the float32
inputs: NumPy's float64 rounds each + - * / and sqrt once, exactly as the contract asks (no fma: every product and sum below is its own
array operation).  Three forms that must agree on every row:

``nearest``            all pairs: every query against every reference row.
``nearest_candidates`` for the large sizes: candidates from ``cKDTree.query_ball_point`` at 1.001 r (a superset: the tree's own float64
                       distances are within a few ulp), decided among in the contract's arithmetic.
``nearest_cells``      the 27-cell walk the kernel makes, over a dictionary of cells: what the locality argument of the header claims.

It also makes the cases of tests/test_gpu_map_nearest.py and tests/test_map_nearest_host.py.  Nothing here is a tolerance: the device
result is compared bit for bit."""
import functools

import numpy as np

HALF = 1 << 20
SETTINGS = [(0.25, (0.0, 0.0, 0.0)), (0.3, (0.1, -0.7, 3.3)), (0.1, (0.0, 0.0, 0.0))]
SIZES_SETTING = (0.2, (0.1, -0.7, 3.3))
BAD_ROWS = (11, 23, 31)                # of the random clouds: a NaN row, a row with +inf, a row at 1e7 (out of range at every radius used)
NEG_ZERO_ROW = 5


def parameters(radius, origin):
    """r2, cell and the origin as the build computes them."""
    r = float(np.float32(radius))
    return r * r, r * 1.0009765625, np.array([float(np.float32(x)) for x in origin], np.float64)


def cells(points, cell, o):
    """Per row: in range?, and floor(q) per axis as float64 (junk where out of range)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        q = (p - o) / cell
        g = np.floor(q)
        ok = np.isfinite(q).all(axis=1) & (g >= -HALF + 1).all(axis=1) & (g <= HALF - 2).all(axis=1)
    return ok, g


def _d2(a, b):
    """a (..., 3) against b (..., 3), float64, broadcast: (dx dx + dy dy) + dz dz."""
    with np.errstate(invalid='ignore', over='ignore'):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def _empty(Qa):
    return dict(index=np.full(Qa, -1, np.int32), d2=np.full(Qa, np.inf), count=np.zeros(Qa, np.int32))


def _finish(out):
    out['dist'] = np.sqrt(out['d2']).astype(np.float32)
    return out


def nearest(queries, points, radius, origin, skip_self=False):
    """All pairs.  Returns dict(index (Qa,) int32, dist (Qa,) float32, count (Qa,) int32, d2 (Qa,) float64 -- inf for none)."""
    r2, cell, o = parameters(radius, origin)
    a, b = np.asarray(queries, np.float32).astype(np.float64), np.asarray(points, np.float32).astype(np.float64)
    ok_a, ok_b = cells(queries, cell, o)[0], cells(points, cell, o)[0]
    out = _empty(len(a))
    rows = np.arange(len(b))
    for i in np.nonzero(ok_a)[0]:
        d2 = _d2(a[i], b)
        with np.errstate(invalid='ignore'):
            hit = ok_b & (d2 <= r2)
        if skip_self:
            hit[i] = False
        j = rows[hit]
        if len(j):
            k = np.lexsort((j, d2[j]))[0]                  # smallest (d2, j)
            out['index'][i], out['d2'][i], out['count'][i] = j[k], d2[j[k]], len(j)
    return _finish(out)


def _decide(out, qi, j, a, b, r2, skip_self):
    """Among the candidate pairs (qi[k], j[k]): the contract's decision, vectorised (count per query; the smallest (d2, j) per query)."""
    d2 = _d2(a[qi], b[j])
    hit = d2 <= r2
    if skip_self:
        hit &= qi != j
    qi, j, d2 = qi[hit], j[hit], d2[hit]
    out['count'][:] = np.bincount(qi, minlength=len(a))
    order = np.lexsort((j, d2, qi))
    qi, j, d2 = qi[order], j[order], d2[order]
    first = np.ones(len(qi), bool)
    first[1:] = qi[1:] != qi[:-1]
    out['index'][qi[first]], out['d2'][qi[first]] = j[first], d2[first]
    return _finish(out)


def nearest_candidates(queries, points, radius, origin, skip_self=False):
    """Candidates from a k-d tree over the in-range reference rows at 1.001 r, then the contract's arithmetic."""
    from scipy.spatial import cKDTree
    r2, cell, o = parameters(radius, origin)
    a, b = np.asarray(queries, np.float32).astype(np.float64), np.asarray(points, np.float32).astype(np.float64)
    ok_a, ok_b = cells(queries, cell, o)[0], cells(points, cell, o)[0]
    out = _empty(len(a))
    rows_a, rows_b = np.nonzero(ok_a)[0], np.nonzero(ok_b)[0]
    if not len(rows_a) or not len(rows_b):
        return _finish(out)
    found = cKDTree(b[rows_b]).query_ball_point(a[rows_a], float(np.float32(radius)) * 1.001, return_sorted=False)
    n = np.array([len(f) for f in found])
    qi = np.repeat(rows_a, n)
    j = rows_b[np.concatenate([np.asarray(f, np.int64) for f in found]).astype(np.int64)] if n.sum() else np.zeros(0, np.int64)
    return _decide(out, qi, j, a, b, r2, skip_self)


def nearest_cells(queries, points, radius, origin, skip_self=False):
    """The 27-cell walk over a dictionary of cells."""
    r2, cell, o = parameters(radius, origin)
    a, b = np.asarray(queries, np.float32).astype(np.float64), np.asarray(points, np.float32).astype(np.float64)
    (ok_a, g_a), (ok_b, g_b) = cells(queries, cell, o), cells(points, cell, o)
    members = {}
    for row in np.nonzero(ok_b)[0]:
        members.setdefault(tuple(g_b[row].astype(np.int64)), []).append(row)
    around = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)]
    qi, j = [], []
    for i in np.nonzero(ok_a)[0]:
        g = g_a[i].astype(np.int64)
        for d in around:
            m = members.get((g[0] + d[0], g[1] + d[1], g[2] + d[2]))
            if m:
                qi += [i] * len(m)
                j += m
    return _decide(_empty(len(a)), np.asarray(qi, np.int64), np.asarray(j, np.int64), a, b, r2, skip_self)


def same(got, want):
    """Exact: index and count equal, dist equal as bit patterns."""
    return (np.array_equal(got['index'], want['index']) and np.array_equal(got['count'], want['count'])
            and np.array_equal(np.asarray(got['dist'], np.float32).view(np.uint32), want['dist'].view(np.uint32)))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cloud(Q, seed):
    """Coordinates uniform in +-2; row 5 is -0.0; the bad rows are a NaN row, a row with +inf and a row at 1e7."""
    p = np.random.default_rng(seed).uniform(-2.0, 2.0, (Q, 3)).astype(np.float32)
    if NEG_ZERO_ROW < Q:
        p[NEG_ZERO_ROW] = np.float32(-0.0)
    if Q > max(BAD_ROWS):
        p[BAD_ROWS[0], 1] = np.nan
        p[BAD_ROWS[1], 2] = np.inf
        p[BAD_ROWS[2]] = np.float32(1e7)
    return p


def case_random(Qa=5003, Q=3001):
    """(queries, reference): Qa = 5003 is 20 workgroups, the last one partial."""
    return cloud(Qa, 601), cloud(Q, 602)


@functools.lru_cache(maxsize=None)
def reference_random(setting):
    a, b = case_random()
    return nearest(a, b, *SETTINGS[setting])


LATTICE_R = 0.25
LATTICE_ORIGINS = [(0.0, 0.0, 0.0), (0.125, -0.25, 0.5), (0.001, 0.001, 0.001)]      # the last one 1e-3 off the lattice


@functools.lru_cache(maxsize=None)
def case_lattice(seed=603):
    """Reference: a 12^3 lattice of pitch r = 0.25 (exact in float32) from -1.5, plus every 7th row repeated at the end: ties by row.
    Queries: 375 lattice points, each moved along one axis by exactly r (onto its neighbour: six rows at distance exactly r), by r / 2,
    by r (1 + 1e-7), and by (0.3, 0.3, 0.3)."""
    rng = np.random.default_rng(seed)
    k = np.stack(np.meshgrid(*[np.arange(12)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
    lattice = (k * LATTICE_R - 1.5).astype(np.float32)
    b = np.concatenate([lattice, lattice[::7]])
    picks = lattice[rng.permutation(len(lattice))[:375]].astype(np.float64)
    axis = np.eye(3)[rng.integers(0, 3, 375)] * rng.choice([-1.0, 1.0], 375)[:, None]
    a = np.concatenate([picks + axis * LATTICE_R, picks + axis * (LATTICE_R / 2), picks + axis * (LATTICE_R * (1 + 1e-7)), picks + 0.3])
    return a.astype(np.float32), b


@functools.lru_cache(maxsize=None)
def case_one_cell(seed=604):
    """3000 reference rows in ONE cell of the grid at r = 1 through zero, 256 queries within r of all of them."""
    rng = np.random.default_rng(seed)
    return rng.uniform(0.4, 0.6, (256, 3)).astype(np.float32), rng.uniform(0.4, 0.6, (3000, 3)).astype(np.float32), 1.0, (0.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def case_full_load(Q=4096, seed=605):
    """Q reference rows, each alone in its cell (r = 0.5), in shuffled order: the table of 2 Q slots is exactly half full; Q queries
    spread over the same cells."""
    rng = np.random.default_rng(seed)
    side = 0.5 * 1.0009765625
    at = np.stack(np.unravel_index(rng.permutation(16 ** 3)[:Q], (16, 16, 16)), axis=1) - 8
    b = ((at + rng.uniform(0.05, 0.95, (Q, 3))) * side).astype(np.float32)
    a = (rng.uniform(-8.0, 8.0, (Q, 3)) * side).astype(np.float32)
    return a, b, 0.5, (0.0, 0.0, 0.0)


def case_sizes(Qa, Q):
    return cloud(Qa, 606), cloud(Q, 607)


def case_self(Q=3001):
    """The random reference cloud with row 100 a copy of row 50: against itself, the two find each other at distance 0."""
    p = cloud(Q, 602).copy()
    p[100] = p[50]
    return p


# ---- cloud_metrics as a loop ----------------------------------------------------------------------------------------------------------
def metrics(dist_a, dist_b, radius, threshold):
    """Python floats and integers, row by row."""
    out = {}
    for side, d in (('a', dist_a), ('b', dist_b)):
        n = found = within = 0
        total = clipped = 0.0
        for x in np.asarray(d, np.float32).tolist():
            n += 1
            if x < float("inf"):
                found += 1
                total += x
                clipped += x
            else:
                clipped += float(radius)
            within += x <= float(threshold)
        out.update({'n_' + side: n, 'found_' + side: found, 'within_' + side: within, 'mean_' + side: total / found if found else float("nan"),
                    'clipped_' + side: clipped / n})
    p, r = out['within_a'] / out['n_a'], out['within_b'] / out['n_b']
    out.update(accuracy=out.pop('mean_a'), completion=out.pop('mean_b'), accuracy_clipped=out.pop('clipped_a'),
               completion_clipped=out.pop('clipped_b'), precision=p, recall=r, fscore=2 * p * r / (p + r) if p + r > 0 else 0.0)
    out['chamfer'] = out['accuracy'] + out['completion']
    return out
