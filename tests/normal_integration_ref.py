"""Float64 restatement of the normal-integration definition (DESIGN.md §4 "Normal integration") with numpy / scipy.sparse:
the yardstick of tests/test_normal_integration_host.py and tests/test_gpu_normal_integration.py.  The product never imports it.

Per segment, with u = log z on the mask's pixels, ray = ((c - cx) / fx, (r - cy) / fy, 1) and d = n . ray:
    ax = nx (c - cx) + ny (r - cy) fx / fy + nz fx  (= fx d),    ay = nx (c - cx) fy / fx + ny (r - cy) + nz fy  (= fy d)
    edge (p, q = right neighbour) in the mask: w = (ax_p^2 + ax_q^2) / 2, t = -(ax_p nx_p + ax_q nx_q) / 2   (ay, ny downwards)
    (L u)_p = sum_e w_e (u_p - u_other),   b_q += t,  b_p -= t
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy import ndimage

N0 = np.array([0.22, -0.12, 1.0]) / np.linalg.norm([0.22, -0.12, 1.0])     # plane normal of the curved scene (synth's, unperturbed)


def pixel_coefficients(normals, K):
    """(ax, ay) (H,W) float64."""
    n = np.asarray(normals, dtype=np.float64)
    H, W = n.shape[:2]
    fx, fy, cx, cy = (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    ax = n[..., 0] * (c - cx) + n[..., 1] * (r - cy) * fx / fy + n[..., 2] * fx
    ay = n[..., 0] * (c - cx) * fy / fx + n[..., 1] * (r - cy) + n[..., 2] * fy
    return ax, ay


def build_system(normals, K, mask):
    """(L csr (P,P) float64, b (P,) float64, index (H,W) int: position of a mask pixel among the unknowns in raster order, -1 off
    the mask)."""
    mask = np.asarray(mask, dtype=bool)
    n = np.asarray(normals, dtype=np.float64)
    ax, ay = pixel_coefficients(n, K)
    index = np.full(mask.shape, -1, dtype=np.int64)
    P = int(mask.sum())
    index[mask] = np.arange(P)
    rows, cols, vals = [], [], []
    b = np.zeros(P)
    for a, nn, ep, eq in ((ax, n[..., 0], (slice(None), slice(0, -1)), (slice(None), slice(1, None))),
                          (ay, n[..., 1], (slice(0, -1), slice(None)), (slice(1, None), slice(None)))):
        both = mask[ep] & mask[eq]
        ip, iq = index[ep][both], index[eq][both]
        w = 0.5 * (a[ep][both] ** 2 + a[eq][both] ** 2)
        t = -0.5 * (a[ep][both] * nn[ep][both] + a[eq][both] * nn[eq][both])
        rows += [ip, iq, ip, iq]
        cols += [ip, iq, iq, ip]
        vals += [w, w, -w, -w]
        np.add.at(b, iq, t)
        np.add.at(b, ip, -t)
    if P == 0:
        return sp.csr_matrix((0, 0)), b, index
    if not rows or sum(len(x) for x in rows) == 0:
        return sp.csr_matrix((P, P)), b, index
    L = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(P, P)).tocsr()
    return L, b, index


def component_labels(mask):
    """Label (1..n) of the 4-connected component of every mask pixel, in the unknowns' raster order."""
    lab, _ = ndimage.label(np.asarray(mask, dtype=bool))
    return lab[np.asarray(mask, dtype=bool)]


def remove_component_means(u, labels):
    u = np.asarray(u, dtype=np.float64).copy()
    if u.size:
        cnt = np.bincount(labels)
        mean = np.bincount(labels, weights=u) / np.maximum(cnt, 1)
        u -= mean[labels]
    return u


def direct_solution(L, b, labels):
    """The solution of L u = b with zero mean on every component: one pixel grounded per component, sparse direct solve, means
    removed.  float64."""
    P = b.shape[0]
    if P == 0:
        return np.zeros(0)
    first = np.unique(labels, return_index=True)[1]
    free = np.ones(P, dtype=bool)
    free[first] = False
    u = np.zeros(P)
    if free.any():
        idx = np.nonzero(free)[0]
        u[idx] = spla.spsolve(L[idx][:, idx].tocsc(), b[idx])
    return remove_component_means(u, labels)


def cg(L, b, cg_tol, cg_max_iter, dtype=np.float32):
    """Plain CG from u = 0 in ``dtype``; stops when the recursive residual has |r_k| <= cg_tol |b| or after cg_max_iter iterations.
    Returns (u, iterations, final |r| / |b|)."""
    L = L.astype(dtype)
    b = b.astype(dtype)
    u = np.zeros_like(b)
    r = b.copy()
    p = b.copy()
    rr = dtype(r @ r) if b.size else dtype(0)
    bb = rr
    k = 0
    if not bb > 0:
        return u, 0, 0.0
    stop = dtype(cg_tol) * np.sqrt(bb)
    while k < cg_max_iter and np.sqrt(rr) > stop:
        q = L @ p
        pq = dtype(p @ q)
        if not pq > 0:
            break
        alpha = dtype(rr / pq)
        u += alpha * p
        r -= alpha * q
        rr_new = dtype(r @ r)
        p = r + dtype(rr_new / rr) * p
        rr = rr_new
        k += 1
    return u, k, float(np.sqrt(rr) / np.sqrt(bb))


def scatter(u, index):
    """(H,W) float64 image of the unknowns, NaN off the mask."""
    out = np.full(index.shape, np.nan)
    out[index >= 0] = u
    return out


# ---- analytic surfaces ---------------------------------------------------------------------------------------------
def camera(H, W):
    return np.array([[0.8 * W, 0, W / 2.0], [0, 0.8 * W, H / 2.0], [0, 0, 1.0]])


def curved_scene(H, W):
    """log z = -log(n0 . ray) + g(x~, y~), g = 0.08 sin(11 x~) cos(15 y~) + 0.05 sin(6 (x~ + 2 y~)): (normals (H,W,3) float64 from the
    analytic gradient, K, log z (H,W), mask (H,W): an ellipse with an elliptic hole, both given in x~, y~)."""
    K = camera(H, W)
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y = (c - K[0, 2]) / K[0, 0], (r - K[1, 2]) / K[1, 1]
    d0 = N0[0] * x + N0[1] * y + N0[2]
    g = 0.08 * np.sin(11 * x) * np.cos(15 * y) + 0.05 * np.sin(6 * (x + 2 * y))
    gx = 0.88 * np.cos(11 * x) * np.cos(15 * y) + 0.3 * np.cos(6 * (x + 2 * y))
    gy = -1.2 * np.sin(11 * x) * np.sin(15 * y) + 0.6 * np.cos(6 * (x + 2 * y))
    logz = -np.log(d0) + g
    ux, uy = -N0[0] / d0 + gx, -N0[1] / d0 + gy            # d log z / d x~, d log z / d y~
    # a normal n with u_x~ = -nx / (n . ray), u_y~ = -ny / (n . ray):  n ~ (-u_x~, -u_y~, 1 + u_x~ x~ + u_y~ y~)
    n = np.stack([-ux, -uy, 1.0 + ux * x + uy * y], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    mask = ((x / 0.55) ** 2 + (y / 0.40) ** 2 <= 1.0) & (((x - 0.10) / 0.18) ** 2 + ((y + 0.05) / 0.12) ** 2 > 1.0)
    return n, K, logz, mask


def plane_normal_of_pair(pair):
    """The unit normal of a synth pair's plane (the first draw of make_pair's generator), float64."""
    n = np.array([0.22, -0.12, 1.0]) + 0.05 * np.random.default_rng(pair.meta["seed"]).standard_normal(3)
    return n / np.linalg.norm(n)
