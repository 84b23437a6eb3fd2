"""Float64 restatement of the normal-integration definition (DESIGN.md §4 "Normal integration") with numpy / scipy.sparse:
the yardstick of tests/test_normal_integration_host.py and tests/test_gpu_normal_integration.py.  The product never imports it.
The second half restates the device's stages one by one for tests/test_gpu_normal_integration_pin.py: the plan (``plan_ref``), the vector
layout in the scratch (``vector_views``, a white-box reader), the set-up with its rounding bounds (``weights_and_rhs``) and one CG
iteration on the padded layout (``cg_step``); tests/test_normal_integration_ref_host.py holds that half against the first.

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


def cg(L, b, cg_tol, cg_max_iter, dtype=np.float32, dots=None):
    """Plain CG from u = 0 in ``dtype``; stops when the recursive residual has |r_k| <= cg_tol |b| or after cg_max_iter iterations.
    ``dots``: the type the three dot products are accumulated in before they are rounded to ``dtype`` (default: ``dtype`` itself).
    Returns (u, iterations, final |r| / |b|)."""
    L = L.astype(dtype)
    b = b.astype(dtype)
    wide = dtype if dots is None else dots

    def dot(x, y):
        return dtype(x.astype(wide) @ y.astype(wide))

    u = np.zeros_like(b)
    r = b.copy()
    p = b.copy()
    rr = dot(r, r) if b.size else dtype(0)
    bb = rr
    k = 0
    if not bb > 0:
        return u, 0, 0.0
    stop = dtype(cg_tol) * np.sqrt(bb)
    while k < cg_max_iter and np.sqrt(rr) > stop:
        q = L @ p
        pq = dot(p, q)
        if not pq > 0:
            break
        alpha = dtype(rr / pq)
        u += alpha * p
        r -= alpha * q
        rr_new = dot(r, r)
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


# ---- the device's plan and vector layout, restated (csrc/sp_normals.hip: header comment and the NiSeg record) -------
U32 = 2.0 ** -24                      # unit roundoff of float32
NI_VECS = 6
VECTOR_NAMES = ("wR", "wD", "u", "r", "p", "q")
PLAN_HEAD, SEG_WORDS = 4, 8           # int32 words: {int64 total, two spare}, then N records of 8, then N order entries
NI_LDS_FLOATS = 38912                 # (only to choose shapes on both sides of a tier edge; no expectation depends on it)
SEG_FIELDS = ("r0", "c0", "bh", "bw", "off", "S", "len")


def stride_of(bw):
    return (int(bw) + 15) & ~15


def len_of(bh, bw):
    S = stride_of(bw)
    return ((int(bh) * S + 2 * S + 15) & ~15) if bh > 0 else 0


def plan_words(N):
    return (PLAN_HEAD + (SEG_WORDS + 1) * N + 15) & ~15


def plan_ref(masks, boxes=None):
    """The plan of sp_normal_integration_plan for ``masks`` (N,H,W) and an optional (N,4) hint {row0, col0, row1, col1}:
    dict of int64 arrays r0, c0, bh, bw, off, S, len (N,), ``order`` (N,) and the int ``total``.

    Tight box of the mask's pixels inside the hint clipped to the image (the hint only narrows the scan); an empty mask has
    r0 = c0 = bh = bw = 0.  S = bw rounded up to 16; len = (bh S + 2 S + 15) & ~15, 0 for an empty mask; off = 6 x the sum of len
    over the earlier indices; order = indices by len descending, ties by index; total = 6 x the sum of len."""
    masks = np.asarray(masks).astype(bool)
    N, H, W = masks.shape
    out = {f: np.zeros(N, dtype=np.int64) for f in SEG_FIELDS}
    for n in range(N):
        R0, C0, R1, C1 = 0, 0, H, W
        if boxes is not None:
            R0, C0 = max(int(boxes[n][0]), 0), max(int(boxes[n][1]), 0)
            R1, C1 = min(int(boxes[n][2]), H), min(int(boxes[n][3]), W)
        if R1 <= R0 or C1 <= C0:
            continue
        sub = masks[n, R0:R1, C0:C1]
        rows, cols = np.nonzero(sub.any(1))[0], np.nonzero(sub.any(0))[0]
        if rows.size == 0:
            continue
        out["r0"][n], out["c0"][n] = R0 + rows[0], C0 + cols[0]
        out["bh"][n], out["bw"][n] = rows[-1] - rows[0] + 1, cols[-1] - cols[0] + 1
    for n in range(N):
        out["S"][n] = stride_of(out["bw"][n])
        out["len"][n] = len_of(out["bh"][n], out["bw"][n])
    out["off"][1:] = NI_VECS * np.cumsum(out["len"])[:-1]
    out["order"] = np.array(sorted(range(N), key=lambda n: (-out["len"][n], n)), dtype=np.int64)
    out["total"] = int(NI_VECS * out["len"].sum())
    return out


def read_plan(words, N):
    """The same dict from the int32 words the device wrote (the two spare words and the padding behind ``order`` are not read)."""
    words = np.ascontiguousarray(words, dtype=np.int32)
    rec = words[PLAN_HEAD:PLAN_HEAD + SEG_WORDS * N].reshape(N, SEG_WORDS)
    out = {"r0": rec[:, 0], "c0": rec[:, 1], "bh": rec[:, 2], "bw": rec[:, 3], "S": rec[:, 6], "len": rec[:, 7]}
    out = {k: v.astype(np.int64) for k, v in out.items()}
    out["off"] = np.ascontiguousarray(rec[:, 4:6]).view(np.int64).reshape(N)
    out["order"] = words[PLAN_HEAD + SEG_WORDS * N:PLAN_HEAD + (SEG_WORDS + 1) * N].astype(np.int64)
    out["total"] = int(words[:2].view(np.int64)[0])
    return out


def segment(plan, n):
    """Record n of a plan as a dict of ints."""
    return {f: int(plan[f][n]) for f in SEG_FIELDS}


def vector_views(scratch, plan_words, seg):
    """WHITE-BOX READER of one segment's six vectors in the scratch of sp_normal_integration; it restates the layout that the header
    comment of sp_normals.hip documents and changes with it.  ``scratch``: the whole float32 scratch (plan included), ``plan_words``:
    the plan's length, ``seg``: the segment's record (``segment``).  The vectors wR, wD, u, r, p, q follow one another from float
    plan_words + off, ``len`` floats each; element (row - r0) S + (col - c0) of a vector sits S floats after the vector's first.

    Returns (views, guards): views[name] is the (bh, S) interior, guards[name] = (the S floats in front, everything behind the
    interior up to len).  Views, not copies."""
    S, ln, bh = seg["S"], seg["len"], seg["bh"]
    base = plan_words + seg["off"]
    views, guards = {}, {}
    for v, name in enumerate(VECTOR_NAMES):
        vec = scratch[base + v * ln:base + (v + 1) * ln]
        assert vec.shape[0] == ln, "the scratch ends inside this segment"
        views[name] = vec[S:S + bh * S].reshape(bh, S)
        guards[name] = (vec[:S], vec[S + bh * S:])
    return views, guards


def box_image(img, seg):
    """(bh, S) float64: the segment's box cut out of an (H,W) image, padding columns 0 -- an image on the padded layout."""
    out = np.zeros((seg["bh"], seg["S"]))
    out[:, :seg["bw"]] = np.asarray(img, dtype=np.float64)[seg["r0"]:seg["r0"] + seg["bh"], seg["c0"]:seg["c0"] + seg["bw"]]
    return out


# ---- weights and right-hand side with their rounding bounds ---------------------------------------------------------
AX_OPS = 6      # ax = nx x + (ny y) (fx / fy) + nz fx with x = c - cx, y = r - cy rounded: longest path y (1), ny y (2), fx / fy (1),
#                 their product (2 + 1 + 1 = 4), the two sums (5, 6).  ay the same with the ratio on the first term.
W_OPS = 14      # w = (a_p a_p + a_q a_q) / 2: a product carries both factors' roundings + 1 (13), the sum + 1; halving is exact
H_OPS = 8       # half-sum (a_p n_p + a_q n_q) / 2: product 6 + 0 + 1 (the normal is an input), the sum + 1
B_OPS = 11      # b = up to four half-sums added to an exact 0 one by one: the first addition is exact, three more round


def weights_and_rhs(normals, K, mask):
    """The set-up of one segment in float64 from the float32 inputs the device reads: dict of (H,W) images, 0 off the mask,
        wR, wD     weight of the edge to the right / lower neighbour (0 where that neighbour is not in the mask)
        b          right-hand side: + the half-sums of the right and lower edge, - those of the left and upper edge
        wR_mag, wD_mag, b_mag   the same expressions with every product and term replaced by its absolute value
        wR_bound, wD_bound, b_bound   OPS * 2^-24 * magnitude: what a float32 evaluation in any order may differ by
        ax, ay, ax_mag, ay_mag
    Counts (derived above, rules of se3_ref.py: a product carries the roundings of both factors + 1, a sum those of its worse term
    + 1 relative to the sum of absolute values; contraction to FMA only removes roundings): AX_OPS 6, W_OPS 14, B_OPS 11."""
    mask = np.asarray(mask, dtype=bool)
    assert np.asarray(normals).dtype == np.float32 and np.asarray(K).dtype == np.float32, "bounds are counted from the float32 inputs"
    n = np.asarray(normals, dtype=np.float64)
    H, W = mask.shape
    fx, fy, cx, cy = (float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
    c, r = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    x, y = c - cx, r - cy
    tx = (n[..., 0] * x, n[..., 1] * y * fx / fy, n[..., 2] * fx)
    ty = (n[..., 0] * x * fy / fx, n[..., 1] * y, n[..., 2] * fy)
    out = {"ax": sum(tx), "ay": sum(ty), "ax_mag": sum(np.abs(t) for t in tx), "ay_mag": sum(np.abs(t) for t in ty)}
    b, b_mag = np.zeros((H, W)), np.zeros((H, W))
    for name, a, am, nn, axis in (("wR", out["ax"], out["ax_mag"], n[..., 0], 1), ("wD", out["ay"], out["ay_mag"], n[..., 1], 0)):
        first = (slice(None), slice(0, -1)) if axis == 1 else (slice(0, -1), slice(None))      # p of an edge
        second = (slice(None), slice(1, None)) if axis == 1 else (slice(1, None), slice(None))  # its q
        both = mask[first] & mask[second]
        w, wm, h, hm = (np.zeros((H, W)) for _ in range(4))
        w[first] = np.where(both, 0.5 * (a[first] ** 2 + a[second] ** 2), 0.0)
        wm[first] = np.where(both, 0.5 * (am[first] ** 2 + am[second] ** 2), 0.0)
        h[first] = np.where(both, 0.5 * (a[first] * nn[first] + a[second] * nn[second]), 0.0)
        hm[first] = np.where(both, 0.5 * (am[first] * np.abs(nn[first]) + am[second] * np.abs(nn[second])), 0.0)
        out[name], out[name + "_mag"], out[name + "_bound"] = w, wm, W_OPS * U32 * wm
        b += h
        b[second] -= h[first]
        b_mag += hm
        b_mag[second] += hm[first]
    out["b"], out["b_mag"], out["b_bound"] = b, b_mag, B_OPS * U32 * b_mag
    return out


# ---- one CG iteration on the padded layout --------------------------------------------------------------------------
Q_OPS = 5       # q = four terms w (p_c - p_x): difference 1, product 2, three more sums 5 (the weights and p are the step's inputs)
DOT_EXTRA = 22  # a sum of n float32 terms in any order: at most n - 1 additions + 1 product on a path; the device's own order adds the
#                 6 butterfly levels and the 16 wave partials to a lane's chain -- (n + 22) 2^-24 sum |terms| covers every such order


def dot_bound(n, mag):
    return (n + DOT_EXTRA) * U32 * mag


def cg_step(wR, wD, u, r, p, layout, b_norm=1.0):
    """One CG iteration in float64 from the state (u, r, p) with the weights (wR, wD), all given ON THE PADDED LAYOUT: (bh, S) arrays,
    ``layout`` = (bh, S).  The stencil is the flat one of the device's layout: with S zeros in front and behind, element i uses
    i + 1 (weight wR[i]), i + S (wD[i]), i - 1 (wR[i - 1]) and i - S (wD[i - S]); rows are kept apart by zero weights alone.
    Needs p . L p > 0.  Returns a namespace with
        q, alpha, u, r, beta, p    (the new u, r, p), res = |r'| / b_norm
        q_mag = sum w |p_c - p_x|;  pq, rr, rr_new and their sums of absolute terms pq_mag, rr_mag, rr_new_mag;  n = bh S."""
    from types import SimpleNamespace
    bh, S = layout
    cells = bh * S

    def flat(a):
        z = np.zeros(cells + 2 * S)
        z[S:S + cells] = np.asarray(a, dtype=np.float64).reshape(cells)
        return z

    wr, wd, pp = flat(wR), flat(wD), flat(p)
    i = np.arange(S, S + cells)
    pc = pp[i]
    q, q_mag = np.zeros(cells), np.zeros(cells)
    for w, px in ((wr[i], pp[i + 1]), (wd[i], pp[i + S]), (wr[i - 1], pp[i - 1]), (wd[i - S], pp[i - S])):
        q += w * (pc - px)
        q_mag += np.abs(w) * np.abs(pc - px)
    u0, r0 = (np.asarray(a, dtype=np.float64).reshape(cells) for a in (u, r))
    pq, rr = float(pc @ q), float(r0 @ r0)
    alpha = rr / pq
    u1 = u0 + alpha * pc
    r1 = r0 - alpha * q
    rr_new = float(r1 @ r1)
    beta = rr_new / rr
    p1 = r1 + beta * pc
    sh = (bh, S)
    return SimpleNamespace(q=q.reshape(sh), q_mag=q_mag.reshape(sh), alpha=alpha, u=u1.reshape(sh), r=r1.reshape(sh), beta=beta,
                           p=p1.reshape(sh), res=float(np.sqrt(rr_new)) / b_norm, pq=pq, rr=rr, rr_new=rr_new,
                           pq_mag=float(np.abs(pc) @ np.abs(q)), rr_mag=rr, rr_new_mag=rr_new, n=cells)


def clamp_scene():
    """A chain whose log-depth leaves +-15: one row of 20 pixels at columns 8..27, fx = fy = 100, cx = 19.5, normals with ny = 0 and
    (nx, nz) = (cos t, sin t) solving nx (c - cx) + nz fx = 0.4, so that every ax is 0.4, every weight 0.16 and every step of u about
    -nx / 0.4 = -2.5.  (normals (3,40,3) f32, K (3,3) f32, mask (3,40) bool)."""
    H, W = 3, 40
    K = np.array([[100.0, 0, 19.5], [0, 100.0, 1.0], [0, 0, 1]], dtype=np.float32)
    c = np.arange(W, dtype=np.float64)
    A, B = c - 19.5, 100.0
    t = np.arctan2(B, A) - np.arccos(0.4 / np.hypot(A, B))          # A cos t + B sin t = 0.4, the root with cos t > 0
    normals = np.zeros((H, W, 3))
    normals[..., 0], normals[..., 2] = np.cos(t), np.sin(t)
    mask = np.zeros((H, W), dtype=bool)
    mask[1, 8:28] = True
    return normals.astype(np.float32), K, mask
