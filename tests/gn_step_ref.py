"""Float64 yardstick of ONE per-pair Gauss-Newton / Levenberg-Marquardt call (sp_pairs_gn_step, sp_pairs_gn_step_conv, an iteration of
sp_pairs_schedule_gn_step) and of one SP_PHASE_ADAM iteration, written from the contract in include/sp_hip.h -- numpy, no GPU.

The solver reads nothing but the partial records of the cost pass and a few SpPair fields (kld, pose, seg_tile_off, N, P, tile0,
n_tiles, rec0), so the records here are made by hand (``make_records``) and every branch can be entered on purpose.

Where the device eliminates the log-depths (Schur complement onto the 6x6 pose block, LDL^T, back-substitution), this file builds the
dense damped (6 + N) x (6 + N) system and hands its active part to ``np.linalg.solve``:

    [ H_pp (1 + lam) + 1e-12 I     h_pd              ] [ d_xi ]     [ b_p ]
    [ h_pd^T                       D (1 + lam + damp) ] [ d_d  ] = - [ b_d ]

a segment is an unknown iff its damped diagonal exceeds 1e-12 and the phase moves depths; the pose block is dropped (d_xi = 0) when the
system is not positive definite (with every kept depth diagonal positive that is: when the pose block is not positive definite after
the elimination).  Everything the state holds as float32 is computed in np.float32 here, in the order the header gives.
"""
import numpy as np

NVP = 32          # SP_GN_PARTIAL_FLOATS: span record  [0] sum|r|  [1..21] H_pp upper triangle, row-major  [22..27] b_p  [28] valid points
NVS = 12          # SP_GN_SEG_FLOATS: segment record   [0..5] h_pd  [6] D  [7] b_d  [8] sum|r|  [9] valid points
LM = 8            # SP_LM_STATE_FLOATS
UNUSED = 777.0    # what make_records leaves in the columns nobody may read (span [29..31], segment [10..11])

f32 = np.float32
IU = np.triu_indices(6)


class GnArgs(dict):
    """lm_up, lm_down, lm_min, conv_tol, max_iters, pose_only, depth_damp, next_phase, predicted_exit (+ adam_lr_pose / adam_lr_kld)."""
    __getattr__ = dict.__getitem__

    def __init__(self, **kw):
        super().__init__(lm_up=8.0, lm_down=0.5, lm_min=1e-7, conv_tol=0.0, max_iters=1 << 30, pose_only=False, depth_damp=0.0,
                         next_phase=1, predicted_exit=False, adam_lr_pose=1e-2, adam_lr_kld=1e-3)
        self.update(kw)


def new_state(pose, kld, max_N, lam0=1e-4, scheduled=False):
    """State of a pair before its first call.  ``done`` (sp_pairs_gn_step_conv) or ``phase`` / ``iters`` (schedules) is None when the
    entry point does not have it."""
    lm = np.zeros(LM, f32)
    lm[0], lm[1] = lam0, -1.0
    return dict(pose=np.array(pose, f32).reshape(4, 4), kld=np.array(kld, f32), lm_state=lm,
                backup=np.full(16 + max_N, -5.0, f32), cost=f32(-3.0), done=None if scheduled else 0,
                phase=0 if scheduled else None, iters=0 if scheduled else None, adam=None)


def copy_state(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


# ---------------------------------------------------------------------------------------------------------------------------------
# SE(3)
# ---------------------------------------------------------------------------------------------------------------------------------
def se3_exp(xi):
    """Exp of the twist [tau, phi] as a 4x4 float64 matrix: the matrix exponential of [[phi^, tau], [0, 0]] (tests/se3_ref.py, which holds
    it against mpmath; no private fall-back with a threshold of its own)."""
    from se3_ref import exp_se3          # (imported here: se3_ref imports window_gn_step_ref, which imports this module)
    return exp_se3(np.asarray(xi, np.float64))


def retract(pose, xi):
    """pose <- float32(Exp(xi) pose); the last row is exactly 0 0 0 1."""
    T = (se3_exp(xi) @ np.asarray(pose, np.float64).reshape(4, 4)).astype(f32)
    T[3] = (0, 0, 0, 1)
    return T


# ---------------------------------------------------------------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------------------------------------------------------------
def pair_view(pair):
    """``pair``: dict(N, P, tile0, n_tiles, rec0, seg_tile_off[N + 1])."""
    return int(pair["N"]), int(pair["P"]), int(pair["tile0"]), int(pair["n_tiles"]), int(pair["rec0"]), np.asarray(pair["seg_tile_off"])


def sum_records(span_records, seg_records, pair):
    """The pair's sums in float64 from the STORED float32 records: (sum|r|, H_pp 6x6, b_p, valid points, h_pd N x 6, D, b_d)."""
    N, P, tile0, n_tiles, rec0, sto = pair_view(pair)
    s = np.asarray(span_records, f32).reshape(-1, NVP)[tile0:tile0 + n_tiles].astype(np.float64).sum(0)
    H = np.zeros((6, 6))
    H[IU] = s[1:22]
    H = H + np.triu(H, 1).T
    seg = np.asarray(seg_records, f32).reshape(-1, NVS).astype(np.float64)
    g = np.zeros((N, 8))
    for n in range(N):
        g[n] = seg[rec0 + sto[n]:rec0 + sto[n + 1], :8].sum(0)
    return s[0], H, s[22:28].copy(), s[28], g[:, :6].copy(), g[:, 6].copy(), g[:, 7].copy()


def dense_step(H, bp, h, D, bd, lam, depth_damp=0.0, pose_only=False):
    """(d_xi, d_d clamped to +-0.5, active mask, info) of the damped system above; ``lam`` is the float32 lambda as a float64."""
    N = len(D)
    Dd = D * (1.0 + (float(lam) + float(depth_damp)))
    active = (Dd > 1e-12) & (not pose_only)
    na = int(active.sum())
    A = np.zeros((6 + na, 6 + na))
    A[:6, :6] = H + np.diag(np.diag(H) * float(lam) + 1e-12)
    A[:6, 6:] = h[active].T
    A[6:, :6] = h[active]
    A[6:, 6:] = np.diag(Dd[active])
    rhs = -np.concatenate([bp, bd[active]])
    pose_ok = bool(np.linalg.eigvalsh(A).min() > 0.0)
    dd = np.zeros(N)
    if pose_ok:
        x = np.linalg.solve(A, rhs)
        dxi, dd[active] = x[:6], x[6:]
    else:                       # the pose block is dropped: every kept depth moves by its own Newton step
        dxi = np.zeros(6)
        dd[active] = -bd[active] / Dd[active]
    unclamped = dd.copy()
    dd = np.clip(dd, -0.5, 0.5)
    return dxi, dd, active, dict(cond=float(np.linalg.cond(A)), pose_ok=pose_ok, unclamped=unclamped, matrix=A, rhs=rhs)


def _leave(st, args, spent, on_cap):
    st["phase"], st["iters"] = int(args.next_phase), 0
    st["lm_state"][1] = -1.0
    st["lm_state"][7] = f32(spent if on_cap else -spent)


def gn_step_ref(span_records, seg_records, pair, state, args, info=None):
    """One call on one pair.  Returns the new state (the input is not touched); ``info`` (a dict) receives what was decided:
    decision in {'skip', 'step', 'reject', 'converged'}, and for a step cond / pose_ok / dxi / dd / active / predicted."""
    info = {} if info is None else info
    st = copy_state(state)
    ls = st["lm_state"]
    scheduled = st["phase"] is not None
    if st["done"]:
        info["decision"] = "skip"
        return st
    N, P, *_ = pair_view(pair)
    sr, H, bp, valid, h, D, bd = sum_records(span_records, seg_records, pair)
    cost64 = sr / (3.0 * P)
    cost = f32(cost64)
    last, conv_tol = ls[1], f32(args.conv_tol)
    prev_rejected = ls[4] != 0
    reject = bool(last >= 0 and cost > last * (f32(1) + f32(1e-6)) and not prev_rejected)
    converged = bool(not reject and (scheduled or st["done"] is not None) and conv_tol > 0 and last >= 0 and not prev_rejected
                     and (last - cost) <= conv_tol * last)
    ls[5], ls[6], st["cost"] = cost, f32(valid / P), cost
    if converged:
        info["decision"] = "converged"
        if st["done"] is not None:
            st["done"] = 1
        if scheduled:
            _leave(st, args, st["iters"], False)
            ls[4] = 0
        return st
    if reject:
        info["decision"] = "reject"
        st["pose"] = st["backup"][:16].reshape(4, 4).copy()
        st["kld"] = st["backup"][16:16 + N].copy()
        ls[0] = ls[0] * f32(args.lm_up)
        ls[3] += 1
        ls[4] = 1
        if scheduled:
            n = st["iters"] + 1
            if n >= args.max_iters:
                _leave(st, args, n, True)
                ls[4] = 0
            else:
                st["iters"] = n
        return st
    info["decision"], info["cost"] = "step", cost64
    lam = ls[0]
    if not prev_rejected:
        lam = max(lam * f32(args.lm_down), f32(args.lm_min))
    st["backup"][:16] = st["pose"].ravel()
    st["backup"][16:16 + N] = st["kld"]
    dxi, dd, active, sol = dense_step(H, bp, h, D, bd, lam, f32(args.depth_damp), args.pose_only)
    info.update(sol, dxi=dxi, dd=dd, active=active, lam=float(lam))
    st["kld"] = np.where(active, st["kld"] + dd.astype(f32), st["kld"]).astype(f32)
    st["pose"] = retract(st["pose"], dxi)
    ls[0], ls[1], ls[4] = lam, cost, 0
    ls[2] += 1
    if scheduled:
        n = st["iters"] + 1
        predicted = False
        if args.predicted_exit and conv_tol > 0 and f32(args.depth_damp) == 0 and lam <= f32(1e-2):
            gain = -(bp @ dxi + bd[active] @ dd[active])
            info["gain"] = gain / (3.0 * P)
            predicted = bool(gain / (3.0 * P) <= float(conv_tol) * cost64)
        info["predicted"] = predicted
        if predicted:
            _leave(st, args, n, False)
        elif n >= args.max_iters:
            _leave(st, args, n, True)
        else:
            st["iters"] = n
    return st


def adam_sched_ref(span_records, seg_records, pair, state, args):
    """One SP_PHASE_ADAM iteration: torch.optim.Adam (CPU, float32) on {left pose tangent, log-depths} with the gradient
    float32(b / (3 P)), then the same retraction; never rejected, leaves the phase on its cap.  The optimiser (its moments) lives in
    state['adam'] and is created, with zero moments, by the first call."""
    import torch
    st = copy_state(state)
    ls = st["lm_state"]
    N, P, *_ = pair_view(pair)
    sr, H, bp, valid, h, D, bd = sum_records(span_records, seg_records, pair)
    if st["adam"] is None:
        xi, kld = torch.zeros(6, requires_grad=True), torch.zeros(N, requires_grad=True)
        opt = torch.optim.Adam([dict(params=[xi], lr=float(args.adam_lr_pose)), dict(params=[kld], lr=float(args.adam_lr_kld))],
                               betas=(0.9, 0.999), eps=1e-8)
        st["adam"] = (opt, xi, kld)
    opt, xi, kld = st["adam"]            # (shared with the input state: consecutive calls continue one optimiser, like the device's moments)
    scale = 1.0 / (3.0 * P)
    with torch.no_grad():
        xi.zero_()                       # the tangent is taken at the current pose every iteration
        kld.copy_(torch.from_numpy(st["kld"]))
    xi.grad = torch.from_numpy((bp * scale).astype(f32))
    kld.grad = torch.from_numpy((bd * scale).astype(f32))
    opt.step()
    st["kld"] = kld.detach().numpy().copy()
    st["pose"] = retract(st["pose"], xi.detach().numpy().astype(np.float64))
    cost = f32(sr * scale)
    ls[1], ls[4], ls[5], ls[6], st["cost"] = cost, 0, cost, f32(valid / P), cost
    ls[2] += 1
    n = st["iters"] + 1
    if n >= args.max_iters:
        _leave(st, args, n, True)
    else:
        st["iters"] = n
    return st


def adam_moments(state, max_N):
    """The device layout of the optimiser's state: 2 + 2 (max_N + 8) floats {step, -, m_kld[max_N], v_kld[max_N], m_xi, v_xi, (affine)}."""
    out = np.zeros(2 + 2 * (max_N + 8), f32)
    if state["adam"] is None:
        return out
    opt, xi, kld = state["adam"]
    N = kld.numel()
    out[0] = float(opt.state[xi]["step"])
    out[2:2 + N] = opt.state[kld]["exp_avg"].numpy()
    out[2 + max_N:2 + max_N + N] = opt.state[kld]["exp_avg_sq"].numpy()
    out[2 + 2 * max_N:8 + 2 * max_N] = opt.state[xi]["exp_avg"].numpy()
    out[8 + 2 * max_N:14 + 2 * max_N] = opt.state[xi]["exp_avg_sq"].numpy()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# hand-made records
# ---------------------------------------------------------------------------------------------------------------------------------
def make_records(rng, N, records_per_segment, n_spans, rows_per_record=6, exact=True, residual_scale=1.0, extra_P=3):
    """Mode-1 span and segment records of one pair from drawn per-residual rows {j_pose(6), j_depth, weight, r}.

    records_per_segment: an int or a length-N sequence (0 = a segment without records).  Row k of the pair goes to span k % n_spans
    (spans beyond the number of rows stay all-zero records); a segment's rows are dealt to its records in turn.
    exact: every row entry is a small multiple of 1/4 (weights of 1/2), so every record entry is a multiple of 1/1024 far below 2^16, is
    stored in float32 without rounding, and any float64 sum of records is exact in any order.  Otherwise the entries are normal deviates
    and the float32 store rounds.  The unused columns hold UNUSED.
    Returns dict(span, seg: float32 records; pair: N, P, n_tiles, seg_tile_off; rows: (segment, J[7], w, r) stacked, for lstsq)."""
    rps = np.broadcast_to(np.asarray(records_per_segment, np.int64), (N,))
    sto = np.concatenate([[0], np.cumsum(rps)]).astype(np.int32)
    n_rows = int(rps.sum()) * rows_per_record
    seg_of = np.repeat(np.arange(N), rps * rows_per_record)
    rec_of = np.concatenate([sto[n] + np.arange(rps[n] * rows_per_record) % max(rps[n], 1) for n in range(N)]).astype(np.int64) \
        if n_rows else np.zeros(0, np.int64)
    if exact:
        J = rng.integers(-8, 9, (n_rows, 7)) / 4.0
        J[:, 6] = rng.integers(2, 9, n_rows) / 4.0 * rng.choice([-1.0, 1.0], n_rows)      # (every record carries depth curvature)
        w = rng.integers(1, 5, n_rows) / 2.0
        r = rng.integers(-8, 9, n_rows) / 4.0 * residual_scale
    else:
        J = rng.standard_normal((n_rows, 7))
        J[:, 6] = (0.5 + rng.random(n_rows)) * rng.choice([-1.0, 1.0], n_rows)
        w = 0.5 + rng.random(n_rows)
        r = rng.standard_normal(n_rows) * residual_scale
    span = np.zeros((n_spans, NVP))
    seg = np.zeros((max(int(sto[-1]), 1), NVS))
    span[:, 29:], seg[:, 10:] = UNUSED, UNUSED
    span_of = np.arange(n_rows) % n_spans
    Jp, jd = J[:, :6], J[:, 6]
    outer = (w[:, None, None] * Jp[:, :, None] * Jp[:, None, :])[:, IU[0], IU[1]]
    np.add.at(span[:, 0], span_of, np.abs(r))
    np.add.at(span[:, 1:22], span_of, outer)
    np.add.at(span[:, 22:28], span_of, (w * r)[:, None] * Jp)
    np.add.at(span[:, 28], span_of, 1.0)
    np.add.at(seg[:, 0:6], rec_of, (w * jd)[:, None] * Jp)
    np.add.at(seg[:, 6], rec_of, w * jd * jd)
    np.add.at(seg[:, 7], rec_of, w * jd * r)
    np.add.at(seg[:, 8], rec_of, np.abs(r))
    np.add.at(seg[:, 9], rec_of, 1.0)
    span32, seg32 = span.astype(f32), seg.astype(f32)
    if exact:
        for a, b in ((span, span32), (seg, seg32)):
            assert np.array_equal(a, b.astype(np.float64)) and np.array_equal(a * 1024, np.round(a * 1024)) and np.abs(a).max() < 2 ** 16
    pair = dict(N=N, P=max(n_rows, 1) + extra_P, tile0=0, n_tiles=n_spans, rec0=0, seg_tile_off=sto)
    return dict(span=span32, seg=seg32[:int(sto[-1])], pair=pair, rows=(seg_of, J, w, r))


def set_segment(rec, n, h=None, D=None, bd=None):
    """Overwrite the sums of segment n (it must own a record): the given values go into its first record, its other records give zero."""
    sto = rec["pair"]["seg_tile_off"]
    assert sto[n + 1] > sto[n], "the segment has no record to hold the values"
    cur = rec["seg"][sto[n]:sto[n + 1], :8].astype(np.float64).sum(0)
    new = cur.copy()
    if h is not None:
        new[:6] = h
    if D is not None:
        new[6] = D
    if bd is not None:
        new[7] = bd
    rec["seg"][sto[n]:sto[n + 1], :8] = 0
    rec["seg"][sto[n], :8] = new.astype(f32)


def scale_cost(rec, factor):
    """Scale the pair's sum |r| (span column 0) and nothing else: a scripted cost sequence on one system."""
    rec["span"][:, 0] = (rec["span"][:, 0].astype(np.float64) * factor).astype(f32)


def lstsq_step(rows, N):
    """The minimiser of sum w (J delta + r)^2 over {d_xi, d_d}: the undamped Gauss-Newton step straight from the rows."""
    seg_of, J, w, r = rows
    A = np.zeros((len(r), 6 + N))
    A[:, :6] = J[:, :6]
    A[np.arange(len(r)), 6 + seg_of] = J[:, 6]
    sw = np.sqrt(w)
    x = np.linalg.lstsq(A * sw[:, None], -r * sw, rcond=None)[0]
    return x[:6], x[6:]


def random_pose(rng):
    xi = np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.4, 0.4, 3)])
    return se3_exp(xi).astype(f32)
