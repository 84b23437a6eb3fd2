"""Yardstick of what a scheduled launch does AFTER its per-pair solve (k_pairs_gn_sched in csrc/sp_solver.hip: the verdict, the later
attempts) and of the host loop of sp_pairs_schedule_run, written from the contract in include/sp_hip.h (SpVerdict, SpSchedule, SpQueue,
sp_pairs_schedule_run) -- numpy, no GPU.  It sits on top of gn_step_ref: a pair's state is gn_step_ref's dict with four more keys,

    status    int: what SpVerdict.status holds for the pair (the caller's initial value until a verdict is filed)
    diag      float32[8]: SpVerdict.diag of the pair ([5] zeroed by the caller)
    attempts  int, or None when SpVerdict.attempts is NULL
    evals     int32[SP_MAX_PHASES], or None when SpVerdict.evals is NULL

Everything the device holds as float32 is computed in np.float32 here, one rounding per operation, in the order the header's formulae
give.  Queue runs: which slot a pair lands in depends on timing, so only per-pair results are defined -- each pair's result is what
``run_ref`` gives with all pairs resident.
"""
import numpy as np

import gn_step_ref as ref
from gn_step_ref import f32

NONFINITE, LAST_CAP, DEPTH_RANGE, COST, VALID, SEGMENTS = 1, 2, 4, 8, 16, 32
RETRIED, UNFINISHED, ADAM = 0x100, 0x200, 0x400
SEGMENT_CAP, SEGMENT_POINTS, MIN_SEGMENTS = 2048, 64, 8          # SP_VERDICT_SEGMENTS, _SEGMENT_POINTS, _MIN_SEGMENTS
MAX_PHASES, DIAG_FLOATS = 12, 8
PHASE_POSE_ONLY, PHASE_ADAM, PHASE_PREDICTED_EXIT, DEPTH_DAMP_SHIFT = 1, 8, 16, 8
HUGE = f32(3.0e38)         # a magnitude above this counts as non-finite (NaN, infinity and the last sliver below FLT_MAX)


class Verdict(dict):
    """The scalar fields of SpVerdict; a bound <= 0 is off."""
    __getattr__ = dict.__getitem__

    def __init__(self, **kw):
        super().__init__(kld_bound=0.0, cost_bound=0.0, cost_ratio=0.0, valid_min=0.0, retry_mask=0, lam0=1e-4, seg_max_ratio=0.0,
                         seg_mean_ratio=0.0, seg_product=0.0)
        assert set(kw) <= set(self), set(kw) - set(self)
        self.update(kw)


def sched_info(phases, entry=0, retry_entry=-1, retry2_entry=-1):
    """What the verdict and the host loop read of an SpSchedule: ``phases`` is a list of dict(max_iters, conv_tol, flags, next)."""
    return dict(phases=list(phases), n_phases=len(phases), entry=entry, retry_entry=retry_entry, retry2_entry=retry2_entry)


def with_verdict_state(state, attempts=True, evals=True, status=0, diag_fill=0.0):
    """gn_step_ref's state with the four keys above."""
    st = ref.copy_state(state)
    st["status"], st["diag"] = int(status), np.full(DIAG_FLOATS, diag_fill, f32)
    st["diag"][5] = 0
    st["attempts"] = 0 if attempts else None
    st["evals"] = np.zeros(MAX_PHASES, np.int32) if evals else None
    return st


def phase_args(spec, p, lm=(8.0, 0.5, 1e-7), adam_lr=(1e-2, 1e-3)):
    """gn_step_ref's arguments of phase p (``spec``: dict(max_iters, conv_tol, flags, next))."""
    fl = spec.get("flags", 0)
    return ref.GnArgs(lm_up=lm[0], lm_down=lm[1], lm_min=lm[2], adam_lr_pose=adam_lr[0], adam_lr_kld=adam_lr[1],
                      conv_tol=spec.get("conv_tol", 0.0), max_iters=spec["max_iters"], next_phase=spec.get("next", 0) or p + 1,
                      pose_only=bool(fl & PHASE_POSE_ONLY), depth_damp=0.125 * ((fl >> DEPTH_DAMP_SHIFT) & 0xff),
                      predicted_exit=bool(fl & PHASE_PREDICTED_EXIT), adam=bool(fl & PHASE_ADAM))


# ---------------------------------------------------------------------------------------------------------------------------------
# the within-pair segment test
# ---------------------------------------------------------------------------------------------------------------------------------
def segment_costs(seg_records, pair):
    """float32[min(N, 2048)]: mean |r| of every segment, float32(a / (3 c)) with a = sum of column [8] and c = sum of column [9] over the
    segment's records (float64, in record order); -1 where the segment is not judged (c < 64)."""
    N, _, _, _, rec0, sto = ref.pair_view(pair)
    seg = np.asarray(seg_records, f32).reshape(-1, ref.NVS)
    out = np.full(min(N, SEGMENT_CAP), -1.0, f32)
    for n in range(len(out)):
        a = c = 0.0
        for t in range(int(sto[n]), int(sto[n + 1])):
            a += float(seg[rec0 + t, 8])
            c += float(seg[rec0 + t, 9])
        if c >= SEGMENT_POINTS:
            assert a >= 0.0, "column [8] is a sum of magnitudes"
            out[n] = f32(a / (3.0 * c))
    return out


def rank_median(costs):
    """The judged cost of rank (n_judged - 1) >> 1 when the judged ones (>= 0) are ordered by (value, index); float32(0) below 8 judged."""
    costs = np.asarray(costs, f32)
    idx = np.flatnonzero(costs >= 0)
    if len(idx) < MIN_SEGMENTS:
        return f32(0)
    x = costs[idx]
    want = (len(idx) - 1) >> 1
    rank = ((x[None, :] < x[:, None]) | ((x[None, :] == x[:, None]) & (idx[None, :] < idx[:, None]))).sum(1)
    hit = np.flatnonzero(rank == want)
    assert len(hit) == 1
    return f32(x[hit[0]])


def segment_stats(seg_records, pair):
    """(median, maximum, judged count) of the pair's segment costs: diag[6], diag[7].  The maximum is over every judged segment, also when
    fewer than 8 are judged and there is no median."""
    sc = segment_costs(seg_records, pair)
    judged = sc[sc >= 0]
    return rank_median(sc), (f32(judged.max()) if len(judged) else f32(0)), len(judged)


# ---------------------------------------------------------------------------------------------------------------------------------
# the verdict of a pair that has just left its last phase
# ---------------------------------------------------------------------------------------------------------------------------------
def excursion(kld, kld0):
    """(max |kld - kld0| over the finite differences as float32, whether some difference is not finite)."""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(kld, f32) - np.asarray(kld0, f32))
        fin = d <= HUGE
    return (f32(d[fin].max()) if fin.any() else f32(0)), bool(not fin.all())


def verdict_ref(seg_records, pair, state, kld0, pose0, v, sched, attempt, first_cost):
    """status bits, diag and the retry decision of a pair whose solve has just taken it out of its last phase.

    seg_records: the segment records of the phase it left.  state: after that solve.  kld0 / pose0: the pair's initial values (N, 16).
    v: Verdict.  sched: sched_info.  attempt: attempts[pair], or None when SpVerdict.attempts is NULL.  first_cost: diag[5].
    Returns dict(bits: the SP_STATUS_* tests that fired; again: 0 = the verdict is filed, 1 / 2 = the pair restarts at retry_entry /
    retry2_entry; status: what is filed (bits + RETRIED / ADAM), None when again; diag: float32[8] as filed ([5] = first_cost))."""
    N = ref.pair_view(pair)[0]
    ls = state["lm_state"]
    cost, first = f32(ls[5]), f32(first_cost)
    dmax, bad = excursion(state["kld"][:N], np.asarray(kld0, f32)[:N])
    with np.errstate(all="ignore"):
        bad = bad or not bool((np.abs(np.asarray(state["pose"], f32).ravel()[:12]) <= HUGE).all())
        seg_med, seg_max, _ = segment_stats(seg_records, pair)
        bits = 0
        if bad or not np.abs(cost) <= HUGE:
            bits |= NONFINITE
        if ls[7] > 0:
            bits |= LAST_CAP
        if f32(v.kld_bound) > 0 and dmax > f32(v.kld_bound):
            bits |= DEPTH_RANGE
        if (f32(v.cost_bound) > 0 and cost > f32(v.cost_bound)) or (f32(v.cost_ratio) > 0 and first > 0 and cost > f32(v.cost_ratio) * first):
            bits |= COST
        if f32(v.valid_min) > 0 and f32(ls[6]) < f32(v.valid_min):
            bits |= VALID
        if seg_med > 0 and ((f32(v.seg_max_ratio) > 0 and seg_max > f32(v.seg_max_ratio) * seg_med)
                            or (f32(v.seg_mean_ratio) > 0 and cost > f32(v.seg_mean_ratio) * seg_med)
                            or (f32(v.seg_product) > 0 and (cost / seg_med - f32(1)) * (seg_max / seg_med) > f32(v.seg_product))):
            bits |= SEGMENTS
    at = 2 if attempt is None else int(attempt)
    failed = (bits & int(v.retry_mask)) != 0
    has1, has2 = 0 <= sched["retry_entry"] < sched["n_phases"], 0 <= sched["retry2_entry"] < sched["n_phases"]
    again = 1 if (failed and at == 0 and has1) else 2 if (failed and at <= 1 and has2) else 0
    counted = attempt is not None
    status = None if again else bits | (RETRIED if at > 0 and counted else 0) | (ADAM if at > 1 and counted else 0)
    diag = np.array([cost, dmax, ls[6], abs(ls[7]), at + 1 if counted else 1, first, seg_med, seg_max], f32)
    return dict(bits=bits, again=again, status=status, diag=diag)


def restart_ref(state, sched, again, v, kld0, pose0):
    """What a retried pair holds afterwards: pose / kld bitwise the initial ones (all 16 pose entries, the pair's N log-depths),
    lm_state[0, 1, 4, 7] = {lam0, -1, 0, 0} with [2, 3] (the iteration counts) and [5, 6] (the last evaluated cost and valid fraction)
    kept, iters = 0, phase = the attempt's entry, diag[5] = 0, attempts = again, zero Adam moments; status, the rest of diag, backup,
    cost and evals untouched."""
    st = ref.copy_state(state)
    N = len(st["kld"])
    st["kld"] = np.array(np.asarray(kld0, f32)[:N], f32)
    st["pose"] = np.array(pose0, f32).reshape(4, 4)
    ls = st["lm_state"]
    ls[0], ls[1], ls[4], ls[7] = f32(v.lam0), -1.0, 0.0, 0.0
    st["iters"], st["phase"] = 0, int(sched["retry_entry"] if again == 1 else sched["retry2_entry"])
    st["diag"][5] = 0
    st["attempts"] = again
    st["adam"] = None
    return st


def schedule_step_ref(recs_of_phase, state, sched, v, kld0, pose0, lm=(8.0, 0.5, 1e-7), adam_lr=(1e-2, 1e-3), idle_mask=0, info=None):
    """One launch of k_pairs_gn_sched for one pair.  recs_of_phase(p) -> dict(span, seg, pair): the records phase p reads.  v: Verdict, or
    None for a launch without one (SpVerdict.status NULL: neither the capture nor the verdict happens).  Returns the new state."""
    info = {} if info is None else info
    ph = state["phase"]
    if ph >= sched["n_phases"] or ph < 0:
        info["decision"] = "finished"
        return ref.copy_state(state)
    if (idle_mask >> ph) & 1:
        info["decision"] = "idle"
        return ref.copy_state(state)
    r, a = recs_of_phase(ph), phase_args(sched["phases"][ph], ph, lm, adam_lr)
    if a.get("adam"):
        info["decision"] = "adam"
        st = ref.adam_sched_ref(r["span"], r["seg"], r["pair"], state, a)
    else:
        st = ref.gn_step_ref(r["span"], r["seg"], r["pair"], state, a, info)
    if st.get("evals") is not None:
        st["evals"][ph] += 1
    if v is None:
        return st
    if st["diag"][5] == 0:                       # the cost a pair's attempt starts from; a first cost of exactly 0 is taken again next time
        st["diag"][5] = st["cost"]
    if st["phase"] < sched["n_phases"]:
        return st
    out = verdict_ref(r["seg"], r["pair"], st, kld0, pose0, v, sched, st["attempts"], st["diag"][5])
    info["verdict"] = out
    if out["again"]:
        return restart_ref(st, sched, out["again"], v, kld0, pose0)
    st["status"], st["diag"] = int(out["status"]), out["diag"]
    return st


# ---------------------------------------------------------------------------------------------------------------------------------
# the host loop, all pairs resident
# ---------------------------------------------------------------------------------------------------------------------------------
def run_ref(states, step, sched, v, check_every, max_rounds):
    """sp_pairs_schedule_run.  step(i, state, idle_mask) -> the new state of pair i after one launch.  Returns (rounds launched, the poll
    record [min phase, 0, attempts left, n active, occupancy bits] of the last poll -- None without one --, the final states; ``evals``
    are in the states).  A pair in an SP_PHASE_ADAM phase that no pair was seen in at the last poll sits the rounds out until the next."""
    n_ph = sched["n_phases"]
    adam_mask = sum(1 << p for p, s in enumerate(sched["phases"]) if s.get("flags", 0) & PHASE_ADAM)
    may_retry = v is not None and states[0].get("attempts") is not None and int(v.retry_mask) != 0 and (sched["retry_entry"] >= 0 or sched["retry2_entry"] >= 0)
    last_attempt = 2 if sched["retry2_entry"] >= 0 else 1
    states = list(states)
    it, min_phase, occupied, poll = 0, 0, 0xffffffff, None
    while it < max_rounds:
        rounds = min(max_rounds - it, check_every)
        idle = adam_mask & ~occupied
        for _ in range(rounds):
            states = [step(i, s, idle) for i, s in enumerate(states)]
            it += 1
        phases = [s["phase"] for s in states]
        busy = [p for p in phases if 0 <= p < n_ph]
        min_phase = min(phases)
        occupied = 0
        for p in busy:
            occupied |= 1 << p
        left = int(any(may_retry and s["phase"] < n_ph and s["attempts"] < last_attempt for s in states))
        poll = [min_phase, 0, left, len(busy), occupied]
        if min_phase >= n_ph:
            break
    if min_phase < n_ph and v is not None:
        states = [dict(s, status=UNFINISHED) if s["phase"] < n_ph else s for s in states]
    return it, poll, states
