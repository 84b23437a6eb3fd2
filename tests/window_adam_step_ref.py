"""Float64 yardstick of ONE sp_window_step call (the fused SE(3)-Adam window optimiser, csrc/sp_window.hip) and of ONE
sp_pairs_adam_step call (solve_adam, csrc/sp_solve_device.h), written from the contract in include/sp_hip.h -- numpy, no GPU.

Both calls read nothing but the mode-0 partial records of the cost pass, a few SpPair fields (tile0, n_tiles, P, N, rec0, seg_tile_off and
the pose / aff / kld pointers) and small state arrays, so the records are made by hand (``make_adam_records``) and every branch can be
entered on purpose.

Mode-0 layout.  Span record (16 floats): [0] residual sum, [1..3] d/dt, [4..12] d/dR row-major, [13] unused (UNUSED), [14] d/da_trg,
[15] d/db_trg.  Segment record (1 float): d/dkld.  The reader scales every sum by 1 / (3 P).

One window call (``window_adam_step_ref``)
    r_e      the reduced residual of edge e;  loss = sum_e w_e (abs_loss ? |r_e| : r_e);  c_e = w_e sign(r_e) under abs_loss (sign(0) = 0),
             else w_e
    g_left   [g_t ; (A12 - A21, A20 - A02, A01 - A10)],  A = R g_R^T + t g_t^T, (R, t) the edge's pose slot: the gradient with respect to
             xi in P <- Exp(xi) P  (dr = <g_R, [phi]x R> + <g_t, [phi]x t + tau> = tr([phi]x A) + g_t . tau)
    nodes    kind-0 target += c g_left;  source += -c Ad_P^T g_left;  kind-1 target += c <d(Exp(a) X)/da_k, dr/dP> with the derivative in
             float64 (Richardson-extrapolated central differences of the matrix exponential);  affine: target += c (d/da, d/db), source -=
    blocks   block b += sum over the edges with block == b of c (segment sums)
    Adam     gradients cast to float32; torch.optim.Adam arithmetic (betas 0.9 / 0.999, eps 1e-8) on the float32 parameters and moments
             with the step evaluated in float64; bias corrections from the running products in state[6..9], restarted when state[0] == 0.
             Not applied to nodes / blocks without an edge nor to anything with lr = 0.
    fold-in  kind 0: T <- T Exp(-a) in float64, rounded once, when a != 0, then a <- 0; then renormalise_rotation where flags & 1 (also
             for a fixed node or one without an edge).  kind 1 keeps its tangent.
    slots    every edge's pose and aff slot composed from the new nodes (an edge whose SpPair.aff is NULL has no aff slot).
    state    {Adam step count, iterations done, previous loss, converged flag, last loss, -, beta1^t and beta2^t as two doubles, -, -}:
             skip_first = no update on iteration 0; losses[it] for it < max_losses; the rel_tol freeze is decided after the update went
             in; state[2] is written only when rel_tol > 0; state[5, 10, 11] are never written; a frozen call changes nothing.

``adam_bound``: how far a float32 evaluation in torch's operation order may lie from the float64 step -- derived in its docstring.
"""
import numpy as np

from gn_step_ref import se3_exp
from window_gn_step_ref import NODE, adjoint, compose_edge, make_node, random_pose, renormalise_rotation  # noqa: F401  (re-exported)

NVP = 16          # SP_GRAD_PARTIAL_FLOATS
NVS = 1           # SP_GRAD_SEG_FLOATS
STATE = 12
UNUSED = 777.0    # what make_adam_records leaves in column 13
f32 = np.float32
U = 2.0 ** -24    # unit roundoff of float32: one rounding moves a value by at most U times its magnitude (half an ulp)
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
KIND1_DERIV_ULPS = 60     # float32 error of one entry of d(Exp(a) X)/da_k from se3_exp_times on dual numbers, see adam_bound


class AdamArgs(dict):
    """abs_loss, skip_first, rel_tol, max_losses."""
    __getattr__ = dict.__getitem__

    def __init__(self, **kw):
        super().__init__(abs_loss=0, skip_first=0, rel_tol=0.0, max_losses=8)
        self.update(kw)


def set_moments(nd, m=None, v=None, aff_m=None, aff_v=None):
    """Set the Adam moments of a node made by make_node (which presets values no Adam step may meet: v < 0)."""
    for name, val in (("m", m), ("v", v), ("aff_m", aff_m), ("aff_v", aff_v)):
        if val is not None:
            nd[name] = val
    return nd


def new_state(nodes, klds, bm, bv, pose_slots, aff_slots, t=0, losses_len=11, sentinel=-5.0):
    """State of a window before its first call; t = Adam steps already taken (the running products are preloaded to match)."""
    st = np.zeros(STATE, f32)
    st[0] = t
    st[6:10] = np.array([BETA1 ** t, BETA2 ** t]).view(f32)
    return dict(nodes=np.array(nodes, NODE), klds=[np.array(k, f32) for k in klds], bm=[np.array(k, f32) for k in bm],
                bv=[np.array(k, f32) for k in bv], pose=np.array(pose_slots, f32).reshape(-1, 16), aff=np.array(aff_slots, f32).reshape(-1, 4),
                state=st, losses=np.full(losses_len, sentinel, f32))


def copy_state(s):
    return {k: ([x.copy() for x in v] if isinstance(v, list) else v.copy()) for k, v in s.items()}


def running_products(state):
    return state[6:10].copy().view(np.float64)


# ---------------------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------------------
def make_adam_records(rng, N, records_per_segment, n_tiles, exact=True, grad_scale=1.0, residual=None, P=None, poison=UNUSED):
    """Mode-0 span and segment records of ONE edge / pair.  records_per_segment: an int or a length-N sequence (0 = a segment without
    records).  exact: every entry is a multiple of grad_scale / 4 (grad_scale a power of two) below 2^12 of it, so any float64 sum of
    them is exact in any order.  residual: None = drawn; a number = the residual SUM over the tiles is exactly that (dyadic) value.
    Returns dict(span, seg: float32; pair: N, P, tile0 = 0, n_tiles, rec0 = 0, seg_tile_off)."""
    rps = np.broadcast_to(np.asarray(records_per_segment, np.int64), (N,))
    sto = np.concatenate([[0], np.cumsum(rps)]).astype(np.int32)
    n_rec = int(sto[-1])
    if exact:
        span = rng.integers(-8, 9, (n_tiles, NVP)) / 4.0 * grad_scale
        seg = rng.integers(-8, 9, (n_rec, NVS)) / 4.0 * grad_scale
        span[:, 0] = rng.integers(1, 9, n_tiles) / 4.0 * grad_scale
    else:
        span = rng.standard_normal((n_tiles, NVP)) * grad_scale
        seg = rng.standard_normal((n_rec, NVS)) * grad_scale
        span[:, 0] = (0.25 + rng.random(n_tiles)) * grad_scale
    if residual is not None:
        span[-1, 0] = residual - span[:-1, 0].sum()
        assert span[:, 0].sum() == residual or not exact
    span[:, 13] = poison
    span32, seg32 = span.astype(f32), seg.astype(f32)
    if exact:
        assert np.array_equal(np.delete(span, 13, 1), np.delete(span32, 13, 1).astype(np.float64)) and np.array_equal(seg, seg32.astype(np.float64))
    pair = dict(N=N, P=int(P if P is not None else 3 + 2 * n_tiles + n_rec), tile0=0, n_tiles=n_tiles, rec0=0, seg_tile_off=sto)
    return dict(span=span32, seg=seg32, pair=pair, exact=exact)


def scale_residual(rec, factor):
    """The same records with the residual column times ``factor``: a scripted loss sequence."""
    out = dict(rec, span=rec["span"].copy())
    out["span"][:, 0] = (out["span"][:, 0].astype(np.float64) * factor).astype(f32)
    return out


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


def sums_exact(rec):
    """True when every sum a reader of ``rec`` forms is exact in float64 in ANY order: all entries are multiples of one power of two q and
    the sum of their magnitudes stays below 2^52 q."""
    for a in (np.delete(rec["span"], 13, 1).astype(np.float64), rec["seg"].astype(np.float64)):
        nz = np.abs(a[a != 0])
        if not len(nz):
            continue
        q = 2.0 ** np.floor(np.log2(nz.min()))
        while not np.array_equal(a / q, np.round(a / q)):
            q /= 2
            if q < 2.0 ** -60:
                return False
        if np.abs(a).sum(0).max() / q >= 2.0 ** 52:
            return False
    return True


def reduce_edge(span_records, seg_records, pair):
    """(r, g_t (3), g_R (3x3), d/da, d/db, d/dkld (N)) of one edge: float64 sums of the stored float32 records times 1 / (3 P)."""
    N, P, tile0, n_tiles, rec0, sto = (int(pair["N"]), int(pair["P"]), int(pair["tile0"]), int(pair["n_tiles"]), int(pair["rec0"]),
                                       np.asarray(pair["seg_tile_off"]))
    s = np.asarray(span_records, f32).reshape(-1, NVP)[tile0:tile0 + n_tiles, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 15]].astype(np.float64).sum(0)
    scale = 1.0 / (3.0 * P)
    seg = np.asarray(seg_records, f32).reshape(-1).astype(np.float64)
    dk = np.array([seg[rec0 + sto[n]:rec0 + sto[n + 1]].sum() * scale for n in range(N)])
    s = s * scale
    return s[0], s[1:4], s[4:13].reshape(3, 3), s[13], s[14], dk


def left_gradient(P, g_t, g_R):
    """Gradient of r with respect to xi in P <- Exp(xi) P."""
    P = np.asarray(P, np.float64).reshape(4, 4)
    A = P[:3, :3] @ g_R.T + np.outer(P[:3, 3], g_t)
    return np.concatenate([g_t, [A[1, 2] - A[2, 1], A[2, 0] - A[0, 2], A[0, 1] - A[1, 0]]])


def dexp_times(a, X):
    """d(Exp(a) X)/da_k, k = 0..5, as six 3x4 float64 matrices: central differences at h and h / 2, Richardson-extrapolated (truncation
    ~ h^4, rounding ~ 1e-16 / h: both below 1e-12 at h = 1e-3)."""
    a, X = np.asarray(a, np.float64), np.asarray(X, np.float64).reshape(4, 4)
    out = np.zeros((6, 3, 4))
    for k in range(6):
        d = []
        for h in (1e-3, 5e-4):
            e = np.zeros(6)
            e[k] = h
            d.append(((se3_exp(a + e) - se3_exp(a - e)) @ X)[:3] / (2 * h))
        out[k] = (4 * d[1] - d[0]) / 3
    return out


def window_gradients(span_records, seg_records, win, nodes, pose_slots, abs_loss, T64=None):
    """Float64 loss and gradients of one call (T64: float64 group elements to use instead of the nodes' float32 ones).  Returns dict(r (E), loss, c (E), g6 (n x 6), gaff (n x 2), touched (n), gk [per block],
    named [per block], k1_terms (n x 6): sum_q |c dP_kq rec_q| of the kind-1 targets)."""
    n, E = len(nodes), len(win["edges"])
    g6, gaff, touched, k1 = np.zeros((n, 6)), np.zeros((n, 2)), np.zeros(n, bool), np.zeros((n, 6))
    gk = [np.zeros(int(N)) for N, _ in win["blocks"]]
    named = [False] * len(win["blocks"])
    r, c = np.zeros(E), np.zeros(E)
    loss = 0.0
    dP_of = {}
    for e, (edge, pair) in enumerate(zip(win["edges"], win["pairs"])):
        src, trg, blk, w = int(edge[0]), int(edge[1]), int(edge[2]), float(f32(edge[3]))
        r[e], g_t, g_R, da, db, dk = reduce_edge(span_records, seg_records, pair)
        loss += w * (abs(r[e]) if abs_loss else r[e])
        c[e] = w * np.sign(r[e]) if abs_loss else w
        gl = left_gradient(pose_slots[e], g_t, g_R)
        touched[trg] = True
        if nodes[trg]["kind"] == 0:
            g6[trg] += c[e] * gl
        else:
            if trg not in dP_of:
                dP_of[trg] = dexp_times(nodes[trg]["a"], nodes[trg]["T"] if T64 is None else T64[trg])
            drdP = np.concatenate([g_R, g_t[:, None]], 1)
            terms = dP_of[trg] * drdP[None]
            g6[trg] += c[e] * terms.sum((1, 2))
            k1[trg] += np.abs(c[e] * terms).sum((1, 2))
        gaff[trg] += c[e] * np.array([da, db])
        if src >= 0:
            touched[src] = True
            g6[src] += -c[e] * (adjoint(pose_slots[e]).T @ gl)
            gaff[src] -= c[e] * np.array([da, db])
        gk[blk] += c[e] * dk
        named[blk] = True
    return dict(r=r, loss=loss, c=c, g6=g6, gaff=gaff, touched=touched, gk=gk, named=named, k1_terms=k1)


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------
def adam_step64(g, m0, v0, lr, b1t, b2t):
    """torch.optim.Adam on float32 inputs, evaluated in float64: (m, v, step to ADD); b1t, b2t = beta^t of THIS step."""
    g, m0, v0 = (np.asarray(x, f32).astype(np.float64) for x in (g, m0, v0))
    m = m0 + (1.0 - BETA1) * (g - m0)
    v = BETA2 * v0 + (1.0 - BETA2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - b2t) + EPS
    return m, v, -(float(f32(lr)) / (1.0 - b1t)) * (m / denom)


def adam_float32(g, m0, v0, p0, lr, b1t, b2t):
    """adam_torch of csrc/sp_solve_device.h restated in np.float32, operation by operation (no FMA): (p, m, v)."""
    g, m, v, p0 = (np.asarray(x, f32) for x in (g, m0, v0, p0))
    neg_step, bc2s = f32(-float(f32(lr)) / (1.0 - b1t)), f32(np.sqrt(1.0 - b2t))
    m = m + f32(0.1) * (g - m)
    v = v * f32(0.999)
    v = v + f32(0.001) * g * g
    denom = np.sqrt(v) / bc2s + f32(1e-8)
    return p0 + neg_step * (m / denom), m, v


def adam_bound(g, m0, v0, lr, b1t, b2t, p_new, dg=None):
    """Per-element distance allowed between the float64 step (``adam_step64``, the parameter rounded once) and a float32 evaluation in
    torch's operation order.  Returns (bound on the parameter, on m, on v).

    One float32 rounding moves a value x by at most U |x|, U = 2^-24.  Contraction to FMA only REMOVES roundings, so every count holds
    with or without it.  sqrt and the divisions are allowed 1 ulp = 2 U each (correctly rounded or not).
      m' = m + 0.1f (g - m)             d = g - m: U |d|, worth 0.1 U |d| in m'; 0.1f is off 0.1 by U / 4 and the product rounds: 1.25 U 0.1 |d|;
                                        the add: U |m'|.            E_m = U (0.225 |g - m| + |m'|) + 0.1 dg            (3 operations)
                                        With S_m = max(|m0|, |g|): |g - m| <= 2 S_m, |m'| <= S_m, so E_m <= 1.45 U S_m + 0.1 dg: the moment is
                                        judged at the scale of what went in, not at its own magnitude (m' cancels).
      v' = v 0.999f + 0.001f g g        0.999f is off by 0.22 U, the product rounds: 1.22 U 0.999 v; 0.001f is off by 0.8 U and two products
                                        round: 2.8 U w, w = 0.001 g^2; the add: U v'.
                                        E_v = U (1.22 v + 2.8 w + v') + 0.002 |g| dg  <= 6.1 U S_v + ..., S_v = max(v0, 0.001 g^2)      (4 operations)
      step = ns (m' / (sqrt(v') / bc2s + eps))
                                        relative: sqrt 2 U, bc2s = (float)sqrt(bc2) U, division 2 U, add U, division 2 U, ns = lr (float)(-1 / bc1)
                                        2 U, product U = 11 U; the moments' errors enter as E_m (lr / bc1) / denom and |step| E_v / (2 v')
      p' = p + step                     the device's add and the yardstick's single rounding: half an ulp each = 1 ulp of p'.
    dg is the error of the float32 gradient itself: by default 1 ulp of g (the device's float64 sum may round to the neighbour); for a
    kind-1 node the caller adds the float32 error of se3_exp_times' derivative: KIND1_DERIV_ULPS = 60 ulp per entry -- the 20 ulp
    window_gn_step_ref counts for an entry of Exp(a) X (11 half-ulps per entry of E, three entries and the product sum), times 3 because
    a product of dual numbers rounds three times (two products and an add) where the value rounds once -- at the scale
    sum_q |c dP_kq rec_q| of the sum that forms g_k."""
    g, m0, v0 = (np.asarray(x, f32).astype(np.float64) for x in (g, m0, v0))
    if dg is None:
        dg = 0.0
    dg = np.asarray(dg, np.float64) + np.spacing(np.abs(g).astype(f32)).astype(np.float64) * (g != 0)
    m, v, step = adam_step64(g, m0, v0, lr, b1t, b2t)
    w = (1.0 - BETA2) * g * g
    E_m = U * (0.225 * np.abs(g - m0) + np.abs(m)) + 0.1 * dg
    E_v = U * (1.22 * v0 + 2.8 * w + v) + 0.002 * np.abs(g) * dg
    denom = np.sqrt(v) / np.sqrt(1.0 - b2t) + EPS
    rel_v = np.divide(E_v, 2.0 * v, out=np.zeros_like(v), where=v > 0)
    b_p = 11 * U * np.abs(step) + float(f32(lr)) / (1.0 - b1t) * E_m / denom + np.abs(step) * rel_v
    b_p = b_p + np.spacing(np.abs(np.asarray(p_new, np.float64)).astype(f32)).astype(np.float64)
    return b_p, E_m, E_v


def _adam(info, name, g, m0, v0, p0, lr, b1t, b2t, dg=None):
    """Apply the float64 step to float32 (p0, m0, v0): returns the rounded (p, m, v) and records exact values and bounds under info[name]."""
    g32 = np.asarray(g, np.float64).astype(f32)
    m, v, step = adam_step64(g32, m0, v0, lr, b1t, b2t)
    p = np.asarray(p0, f32).astype(np.float64) + step
    b_p, b_m, b_v = adam_bound(g32, m0, v0, lr, b1t, b2t, p, dg)
    info[name] = dict(g=g32, p=p, m=m, v=v, b_p=b_p, b_m=b_m, b_v=b_v, lr=float(f32(lr)), step=step, p0=np.array(p0, f32), m0=np.array(m0, f32),
                      v0=np.array(v0, f32))
    return p.astype(f32), m.astype(f32), v.astype(f32)


# ---------------------------------------------------------------------------------------------------------------------------------
# one window call
# ---------------------------------------------------------------------------------------------------------------------------------
def window_adam_step_ref(span_records, seg_records, win, state, args, info=None):
    """One call.  win: dict(edges = rows (src_node, trg_node, block, weight), blocks = [(N, lr)], pairs = [dict(N, P, tile0, n_tiles, rec0,
    seg_tile_off)] per edge, no_aff = edges whose SpPair.aff is NULL).  Returns the new state; ``info`` receives decision in {'frozen',
    'skipped', 'step'}, the float64 loss and, for a step, under ('a', i) / ('aff', i) / ('kld', b) the exact parameters, moments and their
    bounds, and under ('T', i) what the tangents' bounds are worth in the folded pose."""
    info = {} if info is None else info
    st = copy_state(state)
    s, nodes = st["state"], st["nodes"]
    if s[3] != 0:
        info["decision"] = "frozen"
        return st
    gr = window_gradients(span_records, seg_records, win, nodes, st["pose"], int(args.abs_loss))
    loss = f32(gr["loss"])
    it = int(s[1])
    upd = not (int(args.skip_first) and it == 0)
    if it < int(args.max_losses):
        st["losses"][it] = loss
    t = s[0]
    b1t, b2t = running_products(s)
    if t == 0:
        b1t, b2t = 1.0, 1.0
    if upd:
        t = t + f32(1)
        b1t, b2t = b1t * BETA1, b2t * BETA2
        s[6:10] = np.array([b1t, b2t]).view(f32)
    done = False
    rel_tol = f32(args.rel_tol)
    if rel_tol > 0:
        with np.errstate(divide="ignore", invalid="ignore"):
            done = bool(it > 0 and np.abs(loss - s[2]) / s[2] < rel_tol)
        s[2] = loss
    s[0], s[1], s[3], s[4] = t, f32(it + 1), f32(1 if done else 0), loss
    info.update(decision="step" if upd else "skipped", loss=gr["loss"], grads=gr, it=it, done=done, t=int(t), b1t=b1t, b2t=b2t)
    if upd:
        for b, (N, lr) in enumerate(win["blocks"]):
            if not (f32(lr) > 0) or not gr["named"][b] or not int(N):
                continue
            st["klds"][b], st["bm"][b], st["bv"][b] = _adam(info, ("kld", b), gr["gk"][b], st["bm"][b], st["bv"][b], st["klds"][b], lr, b1t, b2t)
        for i in range(len(nodes)):
            nd = nodes[i]
            if gr["touched"][i] and nd["lr_pose"] != 0:
                dg = KIND1_DERIV_ULPS * 2 * U * gr["k1_terms"][i] if nd["kind"] == 1 else None
                nd["a"], nd["m"], nd["v"] = _adam(info, ("a", i), gr["g6"][i], nd["m"], nd["v"], nd["a"], nd["lr_pose"], b1t, b2t, dg)
            if gr["touched"][i] and nd["lr_aff"] != 0:
                nd["aff"], nd["aff_m"], nd["aff_v"] = _adam(info, ("aff", i), gr["gaff"][i], nd["aff_m"], nd["aff_v"], nd["aff"], nd["lr_aff"],
                                                            b1t, b2t)
            if nd["kind"] != 0:
                continue
            if nd["a"].any():
                # the tangent the device folds in may differ from this one by its bound b: T Exp(-a) moves by at most sum_k b_k (1 + |a|)
                # per entry in the translation and 2 max_k b_k (1 + |a|) in the rotation (two entries of [d phi]x meet a row of R): 2.02 sum b
                info[("T", i)] = 2.02 * float(np.sum(info[("a", i)]["b_p"])) if ("a", i) in info else 0.0
                Tn = (nd["T"].astype(np.float64).reshape(4, 4) @ se3_exp(-nd["a"].astype(np.float64))).astype(f32)
                Tn[3] = nd["T"][12:]
                nd["T"] = Tn.ravel()
                nd["a"] = 0
            if nd["flags"] & 1:
                nd["T"] = renormalise_rotation(nd["T"])
    compose_all(win, st)
    return st


def compose_all(win, st):
    no_aff = win.get("no_aff", ())
    for e, edge in enumerate(win["edges"]):
        P, af = compose_edge(edge, st["nodes"])
        st["pose"][e] = P.ravel()
        if e not in no_aff:
            st["aff"][e] = af


# ---------------------------------------------------------------------------------------------------------------------------------
# one sp_pairs_adam_step call on one pair
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_state(pose, kld, aff, max_N, step=0, sentinel=-5.0):
    """pose 4x4, kld (N), aff (4) or None, st = the pair's 2 + 2 (max_N + 8) state floats {step count, -, m_kld, v_kld (max_N each), m_xi,
    v_xi (6 each), m_aff, v_aff (2 each)}, zero with the tails of m_kld / v_kld behind N at ``sentinel``."""
    N = len(kld)
    st = np.zeros(2 + 2 * (max_N + 8), f32)
    st[0] = step
    st[2 + N:2 + max_N] = sentinel
    st[2 + max_N + N:2 + 2 * max_N] = sentinel
    return dict(pose=np.array(pose, f32).reshape(4, 4), kld=np.array(kld, f32), aff=None if aff is None else np.array(aff, f32), st=st,
                loss=f32(sentinel))


def pair_adam_step_ref(span_records, seg_records, pair, state, lrs, max_N, info=None):
    """One sp_pairs_adam_step call on one pair: loss = |residual|, up = sign(float32 residual) / (3 P), the left-tangent gradient cast to
    float32, Adam (bias corrections from pow) on kld, on the tangent FROM ZERO and on the target affine pair only, pose <- Exp(step) pose in
    float64 rounded once, st[0] += 1, loss = |float32 residual|.  lrs = (lr_kld, lr_pose, lr_aff)."""
    info = {} if info is None else info
    out = dict(pose=state["pose"].copy(), kld=state["kld"].copy(), aff=None if state["aff"] is None else state["aff"].copy(), st=state["st"].copy())
    N, M = int(pair["N"]), int(max_N)
    r, g_t, g_R, da, db, dk = reduce_edge(span_records, seg_records, pair)
    res = f32(r)
    sg = float(np.sign(res))
    st = out["st"]
    step = st[0] + f32(1)
    b1t, b2t = BETA1 ** float(step), BETA2 ** float(step)
    o = dict(mk=2, vk=2 + M, mx=2 + 2 * M, vx=8 + 2 * M, ma=14 + 2 * M, va=16 + 2 * M)
    out["kld"], st[o["mk"]:o["mk"] + N], st[o["vk"]:o["vk"] + N] = _adam(info, "kld", sg * dk, st[o["mk"]:o["mk"] + N], st[o["vk"]:o["vk"] + N],
                                                                     out["kld"], lrs[0], b1t, b2t)
    gl = left_gradient(state["pose"], sg * g_t, sg * g_R)
    xi, st[o["mx"]:o["mx"] + 6], st[o["vx"]:o["vx"] + 6] = _adam(info, "xi", gl, st[o["mx"]:o["mx"] + 6], st[o["vx"]:o["vx"] + 6], np.zeros(6, f32),
                                                               lrs[1], b1t, b2t)
    T = (se3_exp(xi.astype(np.float64)) @ state["pose"].astype(np.float64)).astype(f32)
    T[3] = (0, 0, 0, 1)
    out["pose"] = T
    info["T"] = 2.02 * float(np.sum(info["xi"]["b_p"]))          # (the left product: the same count as the fold-in's)
    if out["aff"] is not None:
        out["aff"][2:], st[o["ma"]:o["ma"] + 2], st[o["va"]:o["va"] + 2] = _adam(info, "aff", sg * np.array([da, db]), st[o["ma"]:o["ma"] + 2],
                                                                               st[o["va"]:o["va"] + 2], out["aff"][2:], lrs[2], b1t, b2t)
    st[0] = step
    out["loss"] = np.abs(res)
    info.update(residual=r, offsets=o, t=int(step), b1t=b1t, b2t=b2t)
    return out
