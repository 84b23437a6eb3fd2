"""Float64 yardstick of ONE sp_window_gn_step call, written from the contract in include/sp_hip.h (the window graph, the numbering of
the unknowns, the LM state) and the mode-2 record layout -- numpy, no GPU.

The call reads nothing but the partial records of the cost pass, a few SpPair fields (tile0, n_tiles, P, N, rec0, seg_tile_off and the
pose / aff / kld pointers) and the node / edge / block arrays, so the records are made by hand (``make_window_records``) and every branch
can be entered on purpose.

Where the device reduces every edge to a local system over z_e = [xi (6), a, b] and its source block's depths, maps it onto the node
unknowns, eliminates the depths block by block and factors the reduced camera system, this file assembles ONE dense matrix over
[camera unknowns ; free depth rows] through

    z_e = G_e y,   G_e = [ I_8 at the target node | -blockdiag(Ad_P, I_2) at the source node ]      (P = the edge's pose slot)

damps it (camera diagonal x (1 + lambda) + 1e-12, depth diagonal D (1 + lambda), rows with D (1 + lambda) <= 1e-12 removed) and hands it
to ``np.linalg.solve``.  No Schur complement anywhere.  Everything the state holds as float32 is computed in np.float32.

Layout.  Span record (48 floats): [0] sum |r|, [1..21] H_pp upper triangle row-major, [22..27] b_p, [28] valid points, [29..31] H_aa =
{aa, ab, bb}, [32, 33] b_a, [34..39] H_{a,pose}, [40..45] H_{b,pose}, [46, 47] unused.  Segment record (12 floats): [0..5] h_pd, [6] D,
[7] b_d, [8] H_{a,depth}, [9] H_{b,depth}, [10, 11] unused.
"""
import numpy as np

from gn_step_ref import se3_exp

NVP = 48          # SP_GNA_PARTIAL_FLOATS
NVS = 12          # SP_GNA_SEG_FLOATS
STATE = 16
UNUSED = 777.0    # what make_window_records leaves in the columns nobody may read
f32 = np.float32
IU6 = np.triu_indices(6)

# struct SpWindowNode, 176 bytes
NODE = np.dtype([("T", f32, 16), ("a", f32, 6), ("m", f32, 6), ("v", f32, 6), ("aff", f32, 2), ("aff_m", f32, 2), ("aff_v", f32, 2),
                 ("lr_pose", f32), ("lr_aff", f32), ("kind", np.int32), ("flags", np.int32)])
assert NODE.itemsize == 176


class WinArgs(dict):
    """flags, lm_up, lm_down, lm_min, conv_tol, n_unknowns, max_losses."""
    __getattr__ = dict.__getitem__

    def __init__(self, **kw):
        super().__init__(flags=0, lm_up=8.0, lm_down=0.5, lm_min=1e-7, conv_tol=0.0, n_unknowns=0, max_losses=8)
        self.update(kw)


def make_node(T=None, aff=(0.0, 0.0), lr_pose=1.0, lr_aff=1.0, kind=0, flags=0, a=None):
    nd = np.zeros((), NODE)
    nd["T"] = np.eye(4, dtype=f32).ravel() if T is None else np.asarray(T, f32).ravel()
    nd["aff"], nd["lr_pose"], nd["lr_aff"], nd["kind"], nd["flags"] = aff, lr_pose, lr_aff, kind, flags
    nd["m"], nd["v"], nd["aff_m"], nd["aff_v"] = 0.25, 0.5, -0.25, -0.5          # the Adam moments: nobody's business here
    if a is not None:
        nd["a"] = a
    return nd


def new_state(nodes, klds, pose_slots, aff_slots, lam0=2.0, losses_len=12, sentinel=-5.0):
    """State of a window before its first call.  pose_slots / aff_slots: what sp_window_compose left (n_edges x 16 / x 4)."""
    st = np.zeros(STATE, f32)
    st[0], st[1] = lam0, -1.0
    nodes = np.array(nodes, NODE)
    backup = nodes.copy()
    backup.view(f32)[:] = sentinel
    return dict(nodes=nodes, klds=[np.array(k, f32) for k in klds], nodes_backup=backup,
                kld_backup=np.full(sum(len(k) for k in klds), sentinel, f32), pose=np.array(pose_slots, f32).reshape(-1, 16),
                aff=np.array(aff_slots, f32).reshape(-1, 4), state=st, losses=np.full(losses_len, sentinel, f32))


def copy_state(s):
    return {k: ([x.copy() for x in v] if isinstance(v, list) else v.copy()) for k, v in s.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# the graph
# ---------------------------------------------------------------------------------------------------------------------------------
def number_unknowns(nodes):
    """In node order: 6 per node with lr_pose > 0, then 2 per node with lr_aff > 0.  Returns (pose_off, aff_off, n_y); -1 = fixed."""
    pose_off, aff_off, ny = [], [], 0
    for nd in nodes:
        pose_off.append(ny if nd["lr_pose"] > 0 else -1)
        ny += 6 if nd["lr_pose"] > 0 else 0
        aff_off.append(ny if nd["lr_aff"] > 0 else -1)
        ny += 2 if nd["lr_aff"] > 0 else 0
    return pose_off, aff_off, ny


def adjoint(P):
    """Ad of the rigid motion P = [R t]: [tau', phi'] = [[R, [t]x R], [0, R]] [tau, phi]."""
    P = np.asarray(P, np.float64).reshape(4, 4)
    R, t = P[:3, :3], P[:3, 3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ad = np.zeros((6, 6))
    Ad[:3, :3], Ad[:3, 3:], Ad[3:, 3:] = R, tx @ R, R
    return Ad


def edge_map(edge, nodes, P, numbering=None):
    """G_e (8 x n_y): z_e = G_e y.  The target node's unknowns enter with I_8, the source node's with -blockdiag(Ad_P, I_2); fixed parts
    have no column; src_node = -1 has no source columns."""
    pose_off, aff_off, ny = numbering or number_unknowns(nodes)
    src, trg = int(edge[0]), int(edge[1])
    G = np.zeros((8, ny))
    M = np.zeros((8, 8))
    M[:6, :6], M[6:, 6:] = adjoint(P), np.eye(2)
    for node, block in ((trg, np.eye(8)), (src, -M)):
        if node < 0:
            continue
        if pose_off[node] >= 0:
            G[:, pose_off[node]:pose_off[node] + 6] += block[:, :6]
        if aff_off[node] >= 0:
            G[:, aff_off[node]:aff_off[node] + 2] += block[:, 6:]
    return G


def compose_edge(edge, nodes):
    """(pose slot 4x4 float32, aff slot) of an edge from the nodes: inv(T_trg) T_src at zero tangents (kind 0), Exp(a) X (kind-1 target);
    {a_src, b_src, a_trg, b_trg}.  Float64, rounded once."""
    src, trg = int(edge[0]), int(edge[1])
    nt = nodes[trg]
    Tt = nt["T"].astype(np.float64).reshape(4, 4)
    if nt["kind"] == 1:
        P = se3_exp(nt["a"].astype(np.float64)) @ Tt
    else:
        Ts = nodes[src]["T"].astype(np.float64).reshape(4, 4) if src >= 0 else np.eye(4)
        P = np.eye(4)
        P[:3, :3] = Tt[:3, :3].T @ Ts[:3, :3]
        P[:3, 3] = Tt[:3, :3].T @ (Ts[:3, 3] - Tt[:3, 3])
    P = P.astype(f32)
    P[3] = (0, 0, 0, 1)
    sa = nodes[src]["aff"] if src >= 0 else np.zeros(2, f32)
    return P, np.concatenate([sa, nt["aff"]]).astype(f32)


RENORM_OPS = 19       # float32 operations on the longest path of renormalise_rotation below: 3 adds + sqrt, q * q (or a difference), the
#                       division by den, s (4 products, 3 adds, 1 division), an entry (2 products, an add, a product, a subtraction)


def renormalise_rotation(T16):
    """renormalise_rotation of super_primitive_amd/csrc/sp_solve_device.h (the reference's renormalise_se3: R -> best-conditioned quaternion
    -> R), operation by operation in float32."""
    M = np.array(T16, f32).ravel()
    one, two = f32(1), f32(2)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = M[0], M[1], M[2], M[4], M[5], M[6], M[8], M[9], M[10]
    q = [one + m00 + m11 + m22, one + m00 - m11 - m22, one - m00 + m11 - m22, one - m00 - m11 + m22]
    q = [np.sqrt(x) if x > 0 else f32(0) for x in q]
    best = int(np.argmax(q))                  # first maximum
    qb = q[best]
    a, b, c, d, e, f = m21 - m12, m02 - m20, m10 - m01, m10 + m01, m02 + m20, m12 + m21
    cand = [[q[0] * q[0], a, b, c], [a, q[1] * q[1], d, e], [b, d, q[2] * q[2], f], [c, e, f, q[3] * q[3]]][best]
    den = two * max(qb, f32(0.1))
    r, x, y, z = (v / den for v in cand)
    s = two / (r * r + x * x + y * y + z * z)
    M[0], M[1], M[2] = one - s * (y * y + z * z), s * (x * y - z * r), s * (x * z + y * r)
    M[4], M[5], M[6] = s * (x * y + z * r), one - s * (x * x + z * z), s * (y * z - x * r)
    M[8], M[9], M[10] = s * (x * z - y * r), s * (y * z + x * r), one - s * (x * x + y * y)
    return M


# ---------------------------------------------------------------------------------------------------------------------------------
# records -> local systems -> the dense system
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_view(pair):
    return int(pair["N"]), int(pair["P"]), int(pair["tile0"]), int(pair["n_tiles"]), int(pair["rec0"]), np.asarray(pair["seg_tile_off"])


def read_span(s):
    """(sum |r|, H_z 8x8, b_z, valid points) of a summed span record, z = [xi (6), a, b]."""
    H = np.zeros((8, 8))
    H[:6, :6][IU6] = s[1:22]
    H[6, 6], H[6, 7], H[7, 7] = s[29], s[30], s[31]
    H[:6, 6], H[:6, 7] = s[34:40], s[40:46]
    H = H + np.triu(H, 1).T
    return s[0], H, np.concatenate([s[22:28], s[32:34]]), s[28]


def read_seg(g):
    """(c[8] = H_{z,depth}, D, b_d) of a summed segment record."""
    return np.concatenate([g[0:6], g[8:10]]), g[6], g[7]


def edge_system(span_records, seg_records, pair, weight):
    """Edge e's local system from the STORED float32 records, float64 sums scaled by weight / (3 P):
    (loss_e = sum |r| / (3 P), H_z, b_z, c (N x 8), D (N), b_d (N))."""
    N, P, tile0, n_tiles, rec0, sto = pair_view(pair)
    s = np.asarray(span_records, f32).reshape(-1, NVP)[tile0:tile0 + n_tiles].astype(np.float64).sum(0)
    inv3P = 1.0 / (3.0 * P)
    scale = float(weight) * inv3P
    sr, Hz, bz, _ = read_span(s)
    seg = np.asarray(seg_records, f32).reshape(-1, NVS).astype(np.float64)
    c, D, bd = np.zeros((N, 8)), np.zeros(N), np.zeros(N)
    for n in range(N):
        c[n], D[n], bd[n] = read_seg(seg[rec0 + sto[n]:rec0 + sto[n + 1]].sum(0))
    return sr * inv3P, Hz * scale, bz * scale, c * scale, D * scale, bd * scale


def assemble(win, nodes, pose_slots, systems, flags):
    """The undamped system over [y (n_y) ; every block's rows (sum_N)]: (H, b, n_y, free) with free[r] = depth row r may move (its block
    has lr > 0 and neither flags bit 0 nor bit 2 is set).  Rows that may not move stay empty."""
    numbering = number_unknowns(nodes)
    ny = numbering[2]
    Ns = [int(N) for N, _ in win["blocks"]]
    row0 = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    n = ny + int(row0[-1])
    H, b, free = np.zeros((n, n)), np.zeros(n), np.zeros(int(row0[-1]), bool)
    for k, (N, lr) in enumerate(win["blocks"]):
        free[row0[k]:row0[k + 1]] = lr > 0 and not (flags & 5)
    for e, edge in enumerate(win["edges"]):
        _, Hz, bz, c, D, bd = systems[e]
        G = edge_map(edge, nodes, pose_slots[e], numbering)
        H[:ny, :ny] += G.T @ Hz @ G
        b[:ny] += G.T @ bz
        k = int(edge[2])
        if free[row0[k]] if Ns[k] else False:
            rows = ny + np.arange(row0[k], row0[k + 1])
            H[:ny, rows] += G.T @ c.T
            H[rows, :ny] += c @ G
            H[rows, rows] += D
            b[rows] += bd
    return H, b, ny, free


def dense_step(H, b, ny, free, lam):
    """(dy, dd clamped to +-0.5 over ALL depth rows, active mask, info) of the damped system; ``lam`` is the float32 lambda."""
    lam = float(lam)
    d = np.diag(H).copy()
    Dd = d[ny:] * (1.0 + lam)
    active = free & (Dd > 1e-12)
    A = H.copy()
    A[np.arange(ny), np.arange(ny)] = d[:ny] * (1.0 + lam) + 1e-12
    A[ny + np.arange(len(Dd)), ny + np.arange(len(Dd))] = Dd
    keep = np.concatenate([np.arange(ny), ny + np.nonzero(active)[0]]).astype(int)
    A, rhs = A[np.ix_(keep, keep)], -b[keep]
    ok = bool(ny == 0 or np.linalg.eigvalsh(A).min() > 0.0)
    dy, dd = np.zeros(ny), np.zeros(len(Dd))
    unclamped = dd.copy()
    if ok and len(keep):
        x = np.linalg.solve(A, rhs)
        dy, unclamped[active] = x[:ny], x[ny:]
        dd = np.clip(unclamped, -0.5, 0.5)
    gain = -(b[:ny] @ dy) - (b[ny:][active] @ dd[active])
    return dy, dd, active, dict(ok=ok, cond=float(np.linalg.cond(A)) if len(keep) else 1.0, unclamped=unclamped, gain=gain, matrix=A, rhs=rhs)


def window_loss(win, systems):
    """sum_e weight_e loss_e, in edge order."""
    total = 0.0
    for e, edge in enumerate(win["edges"]):
        total += float(f32(edge[3])) * systems[e][0]
    return total


# ---------------------------------------------------------------------------------------------------------------------------------
# one call
# ---------------------------------------------------------------------------------------------------------------------------------
def window_gn_step_ref(span_records, seg_records, win, state, args, info=None):
    """One call.  win: dict(edges = rows (src_node, trg_node, block, weight), blocks = [(N, lr)], pairs = [dict(N, P, tile0, n_tiles, rec0,
    seg_tile_off)] per edge).  Returns the new state; ``info`` receives decision in {'too_many', 'frozen', 'converged', 'reject', 'step',
    'failed'} and, for a step, cond / dy / dd / active / gain / lam / predicted."""
    info = {} if info is None else info
    st = copy_state(state)
    s, nodes = st["state"], st["nodes"]
    flags = int(args.flags)
    _, _, ny = number_unknowns(nodes)
    free_depths = 0 if flags & 5 else sum(int(N) for N, lr in win["blocks"] if lr > 0)
    info["n_y"] = ny
    if ny > int(args.n_unknowns):                       # more camera unknowns than the caller sized for: refuse and freeze
        s[9], s[6] = 1, 1
        info["decision"] = "too_many"
        return st
    if (ny == 0 and free_depths == 0) or s[6] != 0:
        info["decision"] = "frozen"
        return st
    systems = [edge_system(span_records, seg_records, p, e[3]) for p, e in zip(win["pairs"], win["edges"])]
    loss = f32(window_loss(win, systems))
    last, conv_tol, after_reject = s[1], f32(args.conv_tol), s[4] != 0
    reject = bool(last >= 0 and loss > last * (f32(1) + f32(1e-6)) and not after_reject)
    converged = bool(not reject and last >= 0 and not after_reject and conv_tol > 0 and (last - loss) <= conv_tol * last)
    it = int(s[5])
    if it < int(args.max_losses):
        st["losses"][it] = loss
    s[5], s[7] = f32(it + 1), loss
    if converged:
        s[6] = 1
        info["decision"] = "converged"
        return st
    if reject:                                          # the previous step undone: nodes and log-depths from the backups, re-composed
        info["decision"] = "reject"
        s[0] = s[0] * f32(args.lm_up)
        s[3] += 1
        s[4] = 1
        st["nodes"] = st["nodes_backup"].copy()
        off = 0
        for k, kld in enumerate(st["klds"]):
            st["klds"][k] = st["kld_backup"][off:off + len(kld)].copy()
            off += len(kld)
        _compose_all(win, st)
        return st
    lam = s[0]
    if not after_reject:
        lam = max(lam * f32(args.lm_down), f32(args.lm_min))
    s[0], s[1], s[4] = lam, loss, 0
    s[2] += 1
    st["nodes_backup"] = nodes.copy()
    st["kld_backup"] = np.concatenate(st["klds"]).astype(f32)
    H, b, ny, free = assemble(win, nodes, st["pose"], systems, flags)
    dy, dd, active, sol = dense_step(H, b, ny, free, lam)
    info.update(sol, dy=dy, dd=dd, active=active, lam=float(lam), loss=float(loss), H=H, b=b, free=free)
    if not sol["ok"]:
        # a failed factorisation: no unknown moves; lambda is raised, the call is counted in [8] and flagged as rejected-last -- the next call
        # solves the same point again without a convergence test and without lowering lambda; [1] keeps the loss, [2] and [3] stay
        info["decision"] = "failed"
        s[0] = s[0] * f32(args.lm_up)
        s[8] += 1
        s[4] = 1
        s[2] -= 1
        _compose_all(win, st)
        return st
    info["decision"] = "step"
    off = 0
    for k, kld in enumerate(st["klds"]):
        n = len(kld)
        st["klds"][k] = np.where(active[off:off + n], kld + dd[off:off + n].astype(f32), kld).astype(f32)
        off += n
    pose_off, aff_off, _ = number_unknowns(nodes)
    for i in range(len(nodes)):
        nd = nodes[i]
        if aff_off[i] >= 0:
            nd["aff"] = nd["aff"] + dy[aff_off[i]:aff_off[i] + 2].astype(f32)
        if pose_off[i] < 0:
            continue
        d = dy[pose_off[i]:pose_off[i] + 6]
        T = nd["T"].astype(np.float64).reshape(4, 4)
        if nd["kind"] == 0:
            Tn = (T @ se3_exp(-d)).astype(f32)
            Tn[3] = nd["T"][12:]
            nd["T"] = Tn.ravel()
            if nd["flags"] & 1:
                nd["T"] = renormalise_rotation(nd["T"])
        else:
            Tn = (se3_exp(d) @ se3_exp(nd["a"].astype(np.float64)) @ T).astype(f32)
            Tn[3] = nd["T"][12:]
            nd["T"] = Tn.ravel()
            nd["a"] = 0
    info["predicted"] = False
    if (flags & 2) and conv_tol > 0 and float(lam) <= 1e-2:
        info["predicted"] = bool(sol["gain"] <= float(conv_tol) * float(s[7]))
        if info["predicted"]:
            s[6] = 1
    _compose_all(win, st)
    return st


def _compose_all(win, st):
    for e, edge in enumerate(win["edges"]):
        P, af = compose_edge(edge, st["nodes"])
        st["pose"][e], st["aff"][e] = P.ravel(), af


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-made records
# ---------------------------------------------------------------------------------------------------------------------------------
def make_window_records(rng, N, records_per_segment, n_tiles, rows_per_record=4, exact=True, residual_scale=0.25, extra_P=3):
    """Mode-2 span and segment records of ONE edge from drawn per-residual rows {j_z (8) = [j_pose (6), j_a, j_b], j_d, weight, r}: every
    record entry is a sum of weight x products of one row, so every system built from them is positive semi-definite by construction
    (definite with enough rows).

    records_per_segment: an int or a length-N sequence (0 = a segment without records).  Row k goes to span k % n_tiles; a segment's rows
    are dealt to its records in turn.  exact: every row entry is a small multiple of 1/4 (weights of 1/2): every record entry is stored
    in float32 without rounding and any float64 sum of records is exact in any order.  The unused columns hold UNUSED.
    Returns dict(span, seg: float32 records; pair: N, P, tile0 = 0, n_tiles, rec0 = 0, seg_tile_off; rows: (segment, J[9], w, r))."""
    rps = np.broadcast_to(np.asarray(records_per_segment, np.int64), (N,))
    sto = np.concatenate([[0], np.cumsum(rps)]).astype(np.int32)
    n_rows = int(rps.sum()) * rows_per_record
    seg_of = np.repeat(np.arange(N), rps * rows_per_record)
    rec_of = (np.concatenate([sto[n] + np.arange(rps[n] * rows_per_record) % max(rps[n], 1) for n in range(N)]).astype(np.int64)
              if n_rows else np.zeros(0, np.int64))
    if exact:
        J = rng.integers(-8, 9, (n_rows, 9)) / 4.0
        J[:, 8] = rng.integers(2, 9, n_rows) / 4.0 * rng.choice([-1.0, 1.0], n_rows)      # (every record carries depth curvature)
        w = rng.integers(1, 5, n_rows) / 2.0
        r = rng.integers(-8, 9, n_rows) / 4.0 * residual_scale
    else:
        J = rng.standard_normal((n_rows, 9))
        J[:, 8] = (0.5 + rng.random(n_rows)) * rng.choice([-1.0, 1.0], n_rows)
        w = 0.5 + rng.random(n_rows)
        r = rng.standard_normal(n_rows) * residual_scale
    span = np.zeros((n_tiles, NVP))
    seg = np.zeros((max(int(sto[-1]), 1), NVS))
    span[:, 46:], seg[:, 10:] = UNUSED, UNUSED
    span_of = np.arange(n_rows) % n_tiles
    Jp, ja, jb, jd = J[:, :6], J[:, 6], J[:, 7], J[:, 8]
    outer = (w[:, None, None] * Jp[:, :, None] * Jp[:, None, :])[:, IU6[0], IU6[1]]
    for col, val in ((0, np.abs(r)), (28, np.ones(n_rows)), (29, w * ja * ja), (30, w * ja * jb), (31, w * jb * jb), (32, w * r * ja),
                     (33, w * r * jb)):
        np.add.at(span[:, col], span_of, val)
    np.add.at(span[:, 1:22], span_of, outer)
    np.add.at(span[:, 22:28], span_of, (w * r)[:, None] * Jp)
    np.add.at(span[:, 34:40], span_of, (w * ja)[:, None] * Jp)
    np.add.at(span[:, 40:46], span_of, (w * jb)[:, None] * Jp)
    np.add.at(seg[:, 0:6], rec_of, (w * jd)[:, None] * Jp)
    for col, val in ((6, w * jd * jd), (7, w * jd * r), (8, w * jd * ja), (9, w * jd * jb)):
        np.add.at(seg[:, col], rec_of, val)
    span32, seg32 = span.astype(f32), seg.astype(f32)
    if exact:
        for a, b in ((span, span32), (seg, seg32)):
            assert np.array_equal(a, b.astype(np.float64)) and np.array_equal(a * 1024, np.round(a * 1024)) and np.abs(a).max() < 2 ** 16
    pair = dict(N=N, P=max(n_rows, 1) + extra_P, tile0=0, n_tiles=n_tiles, rec0=0, seg_tile_off=sto)
    return dict(span=span32, seg=seg32[:int(sto[-1])], pair=pair, rows=(seg_of, J, w, r))


def set_segment(rec, n, c=None, D=None, bd=None):
    """Overwrite the raw sums of segment n (it must own a record): the values go into its first record, its other records give zero."""
    sto = rec["pair"]["seg_tile_off"]
    assert sto[n + 1] > sto[n], "the segment has no record to hold the values"
    new = rec["seg"][sto[n]:sto[n + 1], :10].astype(np.float64).sum(0)
    if c is not None:
        new[0:6], new[8:10] = c[:6], c[6:]
    if D is not None:
        new[6] = D
    if bd is not None:
        new[7] = bd
    rec["seg"][sto[n]:sto[n + 1], :10] = 0
    rec["seg"][sto[n], :10] = new.astype(f32)


def scale_cost(rec, factor):
    """Scale the edge's sum |r| (span column 0) and nothing else: a scripted loss sequence on one system."""
    rec["span"][:, 0] = (rec["span"][:, 0].astype(np.float64) * factor).astype(f32)


def lay_out(recs, guard=1.0e6, lead=1):
    """The records of every edge in one span and one segment array with a guard record in front of and behind every edge's own (so tile0
    and rec0 are non-zero).  Returns (span, seg, pairs) with each pair's tile0 / rec0 set."""
    spans, segs, pairs = [np.full((lead, NVP), guard, f32)], [np.full((lead, NVS), guard, f32)], []
    t, q = lead, lead
    for r in recs:
        pairs.append(dict(r["pair"], tile0=t, rec0=q))
        spans += [r["span"], np.full((1, NVP), guard, f32)]
        segs += [r["seg"].reshape(-1, NVS), np.full((1, NVS), guard, f32)]
        t += len(r["span"]) + 1
        q += len(r["seg"]) + 1
    return np.concatenate(spans), np.concatenate(segs), pairs


def lstsq_step(win, nodes, pose_slots, recs, flags=0):
    """The minimiser of sum_e (weight_e / (3 P_e)) sum_rows w (j_z . G_e y + j_d dd + r)^2 over [y ; free depth rows]: the undamped
    Gauss-Newton step straight from the rows the records were made from.  Returns (dy, dd over all rows)."""
    numbering = number_unknowns(nodes)
    ny = numbering[2]
    Ns = [int(N) for N, _ in win["blocks"]]
    row0 = np.concatenate([[0], np.cumsum(Ns)]).astype(int)
    rows_A, rows_r = [], []
    for e, (edge, rec) in enumerate(zip(win["edges"], recs)):
        seg_of, J, w, r = rec["rows"]
        k = int(edge[2])
        free = win["blocks"][k][1] > 0 and not (flags & 5)
        A = np.zeros((len(r), ny + row0[-1]))
        A[:, :ny] = J[:, :8] @ edge_map(edge, nodes, pose_slots[e], numbering)
        if free:
            A[np.arange(len(r)), ny + row0[k] + seg_of] = J[:, 8]
        sw = np.sqrt(w * float(f32(edge[3])) / (3.0 * rec["pair"]["P"]))
        rows_A.append(A * sw[:, None])
        rows_r.append(-r * sw)
    A, rr = np.concatenate(rows_A), np.concatenate(rows_r)
    used = np.abs(A).sum(0) > 0
    x = np.zeros(A.shape[1])
    x[used] = np.linalg.lstsq(A[:, used], rr, rcond=None)[0]
    return x[:ny], x[ny:]


def random_pose(rng, scale=1.0):
    xi = np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.4, 0.4, 3)]) * scale
    return se3_exp(xi).astype(f32)
