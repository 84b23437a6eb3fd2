"""The contract of ``sp_cloud_register`` (include/sp_hip.h) restated in float64 NumPy on the float32 inputs: NumPy's float64 rounds each
+ - * / and sqrt once, exactly as the contract asks (no fma: every product and sum below is its own array operation), so the moved
points, the distances, the residuals and the Jacobians are the device's to the bit; the sums over the rows and the solve
(``np.linalg.solve``) are not, and ``sums_of`` returns per entry of H, g and the cost the sum of the |terms| the bounds of the tests
are made of.

The neighbour of a moved point is found by ``cKDTree.query(k=2)`` over the in-range reference rows and decided between the two
candidates in the contract's arithmetic (``map_nearest_ref``'s range test and d2).  That is the grid's answer as long as no decision is
close: ``rows_of`` returns ``gap``, the smallest relative distance of any decision from flipping -- best against second-best d2, and
best d2 against r2 -- and ``check_gap`` asserts it is > 1e-9 (float64 rounding moves d2 by 1e-16 relative) for every case served.

It also makes the clouds of tests/test_gpu_cloud_register.py and tests/test_cloud_register_host.py: samples of a smooth bumpy height
field over [-1, 1]^2 at z about 2 with analytic normals, r = 0.25."""
import functools

import numpy as np

import map_nearest_ref as near

RUNNING, CONVERGED, MAX_ITERS, FEW, DEGENERATE = range(5)
RADIUS, ORIGIN = 0.25, (0.0, 0.0, 0.0)
SMALL_ANGLE2 = 2.0 ** -26
N_H, N_G = 28, 7                               # the upper triangle of 7 x 7, row major; g; then the cost: 36 sums
BAD_ROWS = (11, 23, 31)                        # a NaN row, a row with +inf, a row at 1e7 (out of range)
BAD_NORMAL_ROW = 40                            # a good point whose normal has a NaN


# ---- the surface ------------------------------------------------------------------------------------------------------------------------
def height(x, y):
    """z and the unit normal (facing -z, towards a camera at the origin) of the height field at (x, y), float64."""
    z = 2.0 + 0.15 * np.sin(2.3 * x + 0.4) * np.cos(1.7 * y) + 0.1 * np.sin(3.1 * y - 0.7) + 0.05 * x * y
    zx = 0.15 * 2.3 * np.cos(2.3 * x + 0.4) * np.cos(1.7 * y) + 0.05 * y
    zy = -0.15 * 1.7 * np.sin(2.3 * x + 0.4) * np.sin(1.7 * y) + 0.1 * 3.1 * np.cos(3.1 * y - 0.7) + 0.05 * x
    n = np.stack([zx, zy, -np.ones_like(zx)], axis=-1)
    return z, n / np.sqrt((n * n).sum(axis=-1, keepdims=True))


@functools.lru_cache(maxsize=None)
def samples(Q, seed, bad=False):
    """(points (Q,3), normals (Q,3)) float32: Q uniform samples of the surface; ``bad``: the three bad rows and a NaN normal."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-1.0, 1.0, Q), rng.uniform(-1.0, 1.0, Q)
    z, n = height(x, y)
    p, n = np.stack([x, y, z], axis=1).astype(np.float32), n.astype(np.float32)
    if bad and Q > BAD_NORMAL_ROW:
        p[BAD_ROWS[0], 1] = np.nan
        p[BAD_ROWS[1], 2] = np.inf
        p[BAD_ROWS[2]] = np.float32(1e7)
        n[BAD_NORMAL_ROW, 0] = np.nan
    return p, n


def rodrigues(w):
    """exp([w]x) by the contract's formulas."""
    w = np.asarray(w, np.float64)
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if th2 < SMALL_ANGLE2:
        A, B = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = np.sqrt(th2)
        half = th / 2.0
        h = np.sin(half) / half
        A, B = np.sin(th) / th, 0.5 * h * h
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.empty((3, 3))
    for a in range(3):
        for b in range(3):
            I = 1.0 if a == b else 0.0
            E[a, b] = (I + A * W[a, b]) + B * (w[a] * w[b] - I * th2)
    return E


def move(points, R, t, s):
    """a' of the contract for every row: float64 (Q,3)."""
    a = np.asarray(points, np.float32).astype(np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        return np.stack([s * ((R[k, 0] * a[:, 0] + R[k, 1] * a[:, 1]) + R[k, 2] * a[:, 2]) + t[k] for k in range(3)], axis=1)


def inverse_moved(points, R, t, s):
    """float32(R^T (p - t) / s): the cloud that the similarity (R, t, s) moves back onto ``points`` up to the float32 rounding."""
    p = np.asarray(points, np.float32).astype(np.float64)
    return (((p - t) @ R) / s).astype(np.float32)


TRUTH = dict(R=rodrigues([0.025, -0.02, 0.024]), t=np.array([0.03, -0.028, 0.03]), s=1.02)       # |omega| about 0.04, |t| about 0.05
START = dict(R=rodrigues([0.01, 0.015, -0.012]), t=np.array([0.02, -0.01, 0.015]), s=1.01)


# ---- one iteration ----------------------------------------------------------------------------------------------------------------------
def correspondences(ap, points, radius=RADIUS, origin=ORIGIN):
    """Per moved point the reference row of the contract (-1: none), and the smallest relative margin of any decision."""
    from scipy.spatial import cKDTree
    r2, cell, o = near.parameters(radius, origin)
    b = np.asarray(points, np.float32).astype(np.float64)
    ok_b = near.cells(points, cell, o)[0]
    with np.errstate(invalid='ignore', over='ignore'):
        q = (ap - o) / cell
        g = np.floor(q)
        ok_a = np.isfinite(q).all(axis=1) & (g >= -near.HALF + 1).all(axis=1) & (g <= near.HALF - 2).all(axis=1)
    index = np.full(len(ap), -1, np.int64)
    rows_a, rows_b = np.nonzero(ok_a)[0], np.nonzero(ok_b)[0]
    gap = np.inf
    if len(rows_a) and len(rows_b):
        k = min(2, len(rows_b))
        _, cand = cKDTree(b[rows_b]).query(ap[rows_a], k=k, distance_upper_bound=float(np.float32(radius)) * 1.001)
        cand = cand.reshape(len(rows_a), k)
        d2 = np.full((len(rows_a), 2), np.inf)
        row = np.full((len(rows_a), 2), np.iinfo(np.int64).max)
        for c in range(k):
            have = cand[:, c] < len(rows_b)
            j = rows_b[cand[have, c]]
            d2[have, c], row[have, c] = near._d2(ap[rows_a[have]], b[j]), j
        second = (d2[:, 1] < d2[:, 0]) | ((d2[:, 1] == d2[:, 0]) & (row[:, 1] < row[:, 0]))
        best, other = np.where(second, d2[:, 1], d2[:, 0]), np.where(second, d2[:, 0], d2[:, 1])
        best_row = np.where(second, row[:, 1], row[:, 0])
        hit = best <= r2
        index[rows_a[hit]] = best_row[hit]
        with np.errstate(invalid='ignore', divide='ignore'):
            m = np.isfinite(other)                                                     # (a twin at distance 0 is a tie: margin 0)
            if m.any():
                gap = min(gap, float(np.where(other[m] > 0, (other[m] - best[m]) / np.where(other[m] > 0, other[m], 1.0), 0.0).min()))
            m = np.isfinite(best)
            if m.any():
                gap = min(gap, float((np.abs(best[m] - r2) / r2).min()))
    return index, gap


def rows_of(points, normals, ref_points, ref_normals, R, t, s, kind, with_scale, huber=0.0, radius=RADIUS, origin=ORIGIN):
    """Every row of the residual of every contributing query row: dict(index (Qa,), n, gap, w, r, J (rows,7)) in query-row order (the
    three rows of a point-to-point pair side by side)."""
    ap = move(points, R, t, s)
    index, gap = correspondences(ap, ref_points, radius, origin)
    ok = index >= 0
    with np.errstate(invalid='ignore', over='ignore'):
        ok &= np.isfinite(ap).all(axis=1)
        nrm = None
        if kind == 1:
            nrm = np.asarray(ref_normals, np.float32).astype(np.float64)[np.where(ok, index, 0)]
        elif kind == 2:
            m = np.asarray(normals, np.float32).astype(np.float64)
            ok &= np.isfinite(m).all(axis=1)
            nrm = np.stack([(R[k, 0] * m[:, 0] + R[k, 1] * m[:, 1]) + R[k, 2] * m[:, 2] for k in range(3)], axis=1)
        if nrm is not None:
            ok &= np.isfinite(nrm).all(axis=1)
    index = np.where(ok, index, -1)
    use = np.nonzero(ok)[0]
    p = ap[use]
    b = np.asarray(ref_points, np.float32).astype(np.float64)[index[use]]
    d = p - b
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    zero, one = np.zeros(len(use)), np.ones(len(use))
    if kind == 0:
        rho = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        J = np.stack([np.stack([zero, pz, -py, one, zero, zero, px], axis=1),
                      np.stack([-pz, zero, px, zero, one, zero, py], axis=1),
                      np.stack([py, -px, zero, zero, zero, one, pz], axis=1)], axis=1)                      # (n, 3, 7)
        r = d
    else:
        n = nrm[use]
        nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
        u = p if kind == 1 else b
        ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
        r1 = (nx * d[:, 0] + ny * d[:, 1]) + nz * d[:, 2]
        rho = np.abs(r1)
        J = np.stack([uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx, nx, ny, nz, (nx * px + ny * py) + nz * pz], axis=1)[:, None, :]
        r = r1[:, None]
    w = np.ones(len(use))
    if huber > 0.0:
        with np.errstate(divide='ignore'):
            w = np.where(rho > 0.0, np.minimum(1.0, huber / np.where(rho > 0.0, rho, 1.0)), 1.0)
    if not with_scale:
        J = J.copy()
        J[:, :, 6] = 0.0
    rows = J.shape[1]
    return dict(index=index.astype(np.int32), n=len(use), gap=gap, w=np.repeat(w, rows), r=r.reshape(-1), J=J.reshape(-1, 7))


def sums_of(rows, reverse=False):
    """(sums (36,), sum of |terms| (36,)): H's upper triangle, g, cost -- wJ_a = w J_a, terms wJ_a J_b, wJ_a r, (w r) r."""
    w, r, J = rows['w'], rows['r'], rows['J']
    wJ = w[:, None] * J
    terms = [wJ[:, a] * J[:, b] for a in range(7) for b in range(a, 7)] + [wJ[:, a] * r for a in range(7)] + [(w * r) * r]
    terms = np.stack(terms, axis=1) if len(w) else np.zeros((0, N_H + N_G + 1))
    order = terms[::-1] if reverse else terms
    return order.sum(axis=0), np.abs(terms).sum(axis=0)


def full(upper, m=7):
    """The symmetric m x m matrix of the stored upper triangle of 7 x 7."""
    H = np.zeros((7, 7))
    H[np.triu_indices(7)] = upper
    H = H + np.triu(H, 1).T
    return H[:m, :m]


def retract(R, t, s, delta):
    """(R, t, s) moved on the left by delta = (omega, v, sigma), by the contract's formulas."""
    E = rodrigues(delta[:3])
    e = np.exp(delta[6])
    Rn = np.array([[(E[a, 0] * R[0, b] + E[a, 1] * R[1, b]) + E[a, 2] * R[2, b] for b in range(3)] for a in range(3)])
    tn = np.array([e * ((E[a, 0] * t[0] + E[a, 1] * t[1]) + E[a, 2] * t[2]) + delta[3 + a] for a in range(3)])
    return Rn, tn, s * e


def step_length(delta, m):
    step = 0.0
    for a in range(m):
        step = step + delta[a] * delta[a]
    return float(np.sqrt(step))


def run(points, normals, ref_points, ref_normals, kind, with_scale, R=None, t=None, s=1.0, huber=0.0, tol=1e-6, min_pairs=None, max_iters=30,
        reverse=False, radius=RADIUS, origin=ORIGIN):
    """The whole estimation.  dict(R, t, s, status, iterations, n, cost, history (max_iters,4), index, gap, first: the sums of the first
    iteration -- dict(sums, abs, n, index, delta, H) --, cond: the condition number of the last H that was solved)."""
    R = np.eye(3) if R is None else np.array(R, np.float64)
    t = np.zeros(3) if t is None else np.array(t, np.float64)
    m = 7 if with_scale else 6
    min_pairs = m if min_pairs is None else min_pairs
    history = np.zeros((max_iters, 4))
    status, gap, first, cond, it = RUNNING, np.inf, None, np.nan, 0
    rows = None
    for it in range(max_iters):
        rows = rows_of(points, normals, ref_points, ref_normals, R, t, s, kind, with_scale, huber, radius, origin)
        gap = min(gap, rows['gap'])
        sums, mass = sums_of(rows, reverse)
        H, g, cost = full(sums[:N_H], m), sums[N_H:N_H + m], sums[N_H + N_G]
        delta, step = np.zeros(7), 0.0
        if rows['n'] < min_pairs:
            status = FEW
        elif not np.isfinite(sums).all() or not _positive_pivots(H):
            status = DEGENERATE
        else:
            delta[:m] = np.linalg.solve(H, -g)
            cond = float(np.linalg.cond(H))
            step = step_length(delta, m)
            R, t, s = retract(R, t, s, delta)
            status = CONVERGED if step <= tol else (MAX_ITERS if it + 1 >= max_iters else RUNNING)
        if first is None:
            first = dict(sums=sums, abs=mass, n=rows['n'], index=rows['index'], delta=delta.copy(), H=H)
        history[it] = (rows['n'], cost, step, status)
        if status != RUNNING:
            break
    history[it + 1:, 3] = status
    return dict(R=R, t=t, s=s, status=status, iterations=it + 1, n=rows['n'], cost=history[it, 1], history=history, index=rows['index'], gap=gap,
                first=first, cond=cond)


def _positive_pivots(H):
    """The pivots of LDL^T in the order the kernel takes them."""
    m = len(H)
    L, d = np.eye(m), np.zeros(m)
    for j in range(m):
        d[j] = H[j, j] - sum(L[j, k] * L[j, k] * d[k] for k in range(j))
        if not d[j] > 0.0:
            return False
        for i in range(j + 1, m):
            L[i, j] = (H[i, j] - sum(L[i, k] * L[j, k] * d[k] for k in range(j))) / d[j]
    return True


def check_gap(out):
    """No decision of the run was within 1e-9 (relative) of flipping: the device cannot have chosen otherwise."""
    assert out['gap'] > 1e-9, f"a correspondence is decided by a relative margin of {out['gap']:.3e}"
    return out


def difference(a, b):
    """The largest |difference| over the entries of R, t and s of two results (dicts with R, t, s)."""
    return max(float(np.abs(np.asarray(a['R']) - np.asarray(b['R'])).max()), float(np.abs(np.asarray(a['t']) - np.asarray(b['t'])).max()),
               abs(float(a['s']) - float(b['s'])))


def rotation_angle(Ra, Rb):
    """The angle of Ra Rb^T (below a right angle), from its skew part: accurate for small angles."""
    v = Ra @ Rb.T
    return float(np.arcsin(min(1.0, np.sqrt((v[2, 1] - v[1, 2]) ** 2 + (v[0, 2] - v[2, 0]) ** 2 + (v[1, 0] - v[0, 1]) ** 2) / 2.0)))


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------
Q_REF, QA_ONE, QA_RUN = 3001, 5003, 2003


def case_one_iteration(Qa=QA_ONE):
    """(queries, query normals, reference, reference normals): independent samples; at Qa = 5003 and Q = 3001 both clouds with a NaN row,
    an inf row, an out-of-range row and a good row with a NaN normal.  The start of these cases is START."""
    a, an = samples(Qa, 701, bad=True)
    b, bn = samples(Q_REF, 702, bad=True)
    return a, an, b, bn


def case_identical():
    """Q = 3001 reference samples; the queries are its first 2003 rows moved back by TRUTH and rounded to float32: the truth is TRUTH."""
    b, bn = samples(Q_REF, 703)
    a = inverse_moved(b[:QA_RUN], TRUTH['R'], TRUTH['t'], TRUTH['s'])
    an = (bn[:QA_RUN].astype(np.float64) @ TRUTH['R']).astype(np.float32)                  # R^T n
    return a, an, b, bn


def case_independent():
    """Independent samples of the surface, the queries moved back by TRUTH."""
    b, bn = samples(Q_REF, 704)
    p, pn = samples(QA_RUN, 705)
    return inverse_moved(p, TRUTH['R'], TRUTH['t'], TRUTH['s']), (pn.astype(np.float64) @ TRUTH['R']).astype(np.float32), b, bn


def case_outliers():
    """Independent samples, the queries moved back by the RIGID part of TRUTH (s = 1: the scale is no unknown of this case -- a plane
    residual with a free scale and one-sided outliers shrinks the cloud), every 20th query then displaced by 0.2 along z."""
    b, bn = samples(Q_REF, 704)
    p, pn = samples(QA_RUN, 705)
    a = inverse_moved(p, TRUTH['R'], TRUTH['t'], 1.0)
    a[::20, 2] += np.float32(0.2)
    return a, (pn.astype(np.float64) @ TRUTH['R']).astype(np.float32), b, bn


def case_lattice():
    """A flat 40 x 40 lattice at z = 2 (pitch 0.05) with normals (0, 0, 1), the queries its points moved by (0.013, 0.007, 0.01): with the
    point-to-plane residual the rotation about z and the translations along x and y have EXACT zero columns."""
    k = np.stack(np.meshgrid(np.arange(40), np.arange(40), indexing='ij'), axis=-1).reshape(-1, 2)
    b = np.concatenate([k * 0.05 - 1.0, np.full((len(k), 1), 2.0)], axis=1).astype(np.float32)
    bn = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (len(b), 1))
    a = (b.astype(np.float64) + np.array([0.013, 0.007, 0.01])).astype(np.float32)
    return a, bn.copy(), b, bn
