"""The reference of the scheduled run's verdict, retries and host loop (tests/schedule_verdict_ref.py) against what include/sp_hip.h says,
on values that can be worked out by hand -- no GPU."""
import itertools

import numpy as np
import pytest

import gn_step_ref as ref
import schedule_verdict_ref as sv
from gn_step_ref import f32

UP, DOWN = 1 + 2.0 ** -9, 1 - 2.0 ** -9          # a threshold moved by 2e-3 of itself, exactly


def seg_pair(costs, points=64.0, records=2):
    """Segment records whose segment n has mean |r| = costs[n] over ``points`` valid points, split over ``records`` records (costs[n] < 0:
    no record)."""
    sto, rows = [0], []
    for c in costs:
        k = 0 if c < 0 else records
        for j in range(k):
            r = np.zeros(ref.NVS, f32)
            r[8], r[9] = 3.0 * points * c / k, points / k
            rows.append(r)
        sto.append(sto[-1] + k)
    pair = dict(N=len(costs), P=100, tile0=0, n_tiles=1, rec0=0, seg_tile_off=np.array(sto, np.int32))
    return np.array(rows, f32).reshape(-1, ref.NVS), pair


def finished_state(N, cost=3.0, valid=0.5, last=-2.0, kld=None):
    st = ref.new_state(np.eye(4), np.ones(N) if kld is None else kld, N + 3, scheduled=True)
    st["lm_state"][5:8] = cost, valid, last
    return sv.with_verdict_state(st)


BASE = [1, 1, 2, 2, 2, 2, 3, 3, 4, 4, 4, 16]           # median (rank 5 of 12) 2, maximum 16


def bits_of(v, costs=BASE, sched=None, attempt=0, first=4.0, **state):
    seg, pair = seg_pair(costs)
    st = finished_state(len(costs), **state)
    return sv.verdict_ref(seg, pair, st, np.ones(len(costs), f32) * 0.75, np.eye(4).ravel(), sv.Verdict(**v), sched or sv.sched_info([dict(max_iters=1)]),
                          attempt, first)


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 12, 13, 64, 301])
def test_rank_median_is_the_lower_median_with_ties(n):
    rng = np.random.default_rng(n)
    for trial in range(20):
        x = rng.integers(0, 5, n).astype(f32) / 4                    # many ties
        x[rng.random(n) < 0.3] = -1                                   # not judged
        judged = x[x >= 0]
        want = np.sort(judged)[(len(judged) - 1) // 2] if len(judged) >= 8 else 0
        assert sv.rank_median(x) == want, (n, trial)


def test_segment_costs_points_floor_and_cap():
    seg, pair = seg_pair([1.0, 2.0, -1, 4.0])
    seg[2, 9] -= 1                                                    # segment 1: 63 points
    assert sv.segment_costs(seg, pair).tolist() == [1.0, -1.0, -1.0, 4.0]
    seg, pair = seg_pair([1.0] * 2047 + [64.0, 128.0], records=1)
    med, mx, n = sv.segment_stats(seg, pair)
    assert (med, mx, n) == (1.0, 64.0, 2048)                          # segment 2048 is not looked at
    med, mx, n = sv.segment_stats(*seg_pair([1, 2, 3, 4, 5, 6, 7]))
    assert (med, mx, n) == (0.0, 7.0, 7)                              # no median below 8 judged segments; the maximum is still reported


# the threshold of every bit: (verdict field, the exactly representable value it ties at, the bit, '>' or '<')
THRESHOLDS = [("kld_bound", 0.25, sv.DEPTH_RANGE, ">"), ("cost_bound", 3.0, sv.COST, ">"), ("cost_ratio", 0.75, sv.COST, ">"), ("valid_min", 0.5, sv.VALID, "<"),
              ("seg_max_ratio", 8.0, sv.SEGMENTS, ">"), ("seg_mean_ratio", 1.5, sv.SEGMENTS, ">"), ("seg_product", 4.0, sv.SEGMENTS, ">")]


@pytest.mark.parametrize("field,tie,bit,sense", THRESHOLDS, ids=[t[0] for t in THRESHOLDS])
def test_each_bit_switches_exactly_at_its_threshold(field, tie, bit, sense):
    # cost 3, first cost 4, valid 0.5, excursion 1 - 0.75, segments BASE: every tested quantity equals its `tie` bound exactly
    flagged, clear = (tie * DOWN, tie * UP) if sense == ">" else (tie * UP, tie * DOWN)
    assert bits_of({field: flagged})["bits"] == bit
    assert bits_of({field: clear})["bits"] == 0
    assert bits_of({field: tie})["bits"] == 0, "a tie is not flagged"
    assert bits_of({field: 0.0})["bits"] == 0 and bits_of({field: -1.0})["bits"] == 0, "a bound <= 0 is off"
    out = bits_of({field: flagged})
    assert out["diag"].tolist() == [3.0, 0.25, 0.5, 2.0, 1.0, 4.0, 2.0, 16.0] and out["status"] == bit and out["again"] == 0


def test_cost_ratio_needs_a_first_cost_and_segments_need_a_median():
    assert bits_of(dict(cost_ratio=0.5), first=0.0)["bits"] == 0
    assert bits_of(dict(seg_max_ratio=2.0), costs=BASE[5:])["bits"] == 0           # 7 judged
    assert bits_of(dict(seg_max_ratio=2.0), costs=BASE[4:])["bits"] == sv.SEGMENTS   # 8


def test_last_cap_and_nonfinite():
    assert bits_of({}, last=2.0)["bits"] == sv.LAST_CAP and bits_of({}, last=-2.0)["bits"] == 0 and bits_of({}, last=0.0)["bits"] == 0
    for bad in (np.nan, np.inf, -np.inf):
        kld = np.ones(12, f32)
        kld[3], kld[7] = bad, 1.5
        out = bits_of({}, kld=kld)
        assert out["bits"] == sv.NONFINITE and out["diag"][1] == 0.75, "dmax is the maximum over the finite entries"
        assert bits_of({}, cost=bad)["bits"] == sv.NONFINITE
    seg, pair = seg_pair(BASE)
    for k in range(16):
        st = finished_state(12)
        st["pose"].reshape(16)[k] = np.inf
        bits = sv.verdict_ref(seg, pair, st, np.ones(12, f32), np.eye(4).ravel(), sv.Verdict(), sv.sched_info([dict(max_iters=1)]), 0, 4.0)["bits"]
        assert bits == (sv.NONFINITE if k < 12 else 0), k                           # the last pose row is not looked at


@pytest.mark.parametrize("has1,has2,attempt,in_mask", list(itertools.product([False, True], [False, True], [0, 1, 2, None], [False, True])))
def test_attempt_table(has1, has2, attempt, in_mask):
    sched = sv.sched_info([dict(max_iters=1)] * 3, entry=2, retry_entry=1 if has1 else -1, retry2_entry=0 if has2 else -1)
    out = bits_of(dict(cost_bound=1.0, retry_mask=sv.COST if in_mask else sv.VALID), sched=sched, attempt=attempt)
    assert out["bits"] == sv.COST
    if not in_mask or attempt is None or attempt == 2:
        again = 0
    elif attempt == 0:
        again = 1 if has1 else 2 if has2 else 0
    else:
        again = 2 if has2 else 0
    assert out["again"] == again
    if again:
        assert out["status"] is None
    else:
        extra = 0 if attempt in (None, 0) else sv.RETRIED if attempt == 1 else sv.RETRIED | sv.ADAM
        assert out["status"] == sv.COST | extra and out["diag"][4] == (1 if attempt is None else attempt + 1)


def test_restart_resets_what_the_header_lists_and_nothing_else():
    st = finished_state(5, kld=np.arange(5) + 2.0)
    st["lm_state"][:] = [0.25, 3.0, 7, 2, 1, 3.0, 0.5, 4]
    st["diag"][:] = [9, 9, 9, 9, 9, 4.0, 9, 9]
    st["status"], st["iters"], st["phase"], st["backup"][:], st["cost"] = -77, 3, 3, 6.0, f32(3.0)
    kld0, pose0 = np.arange(8, dtype=f32), np.arange(16, dtype=f32)
    sched = sv.sched_info([dict(max_iters=1)] * 3, entry=2, retry_entry=1, retry2_entry=0)
    for again, entry in ((1, 1), (2, 0)):
        out = sv.restart_ref(st, sched, again, sv.Verdict(lam0=0.125), kld0, pose0)
        assert out["lm_state"].tolist() == [0.125, -1, 7, 2, 0, 3.0, 0.5, 0] and (out["phase"], out["iters"], out["attempts"]) == (entry, 0, again)
        assert out["kld"].tolist() == [0, 1, 2, 3, 4] and out["pose"].ravel().tolist() == list(range(16)) and out["adam"] is None
        assert out["diag"].tolist() == [9, 9, 9, 9, 9, 0, 9, 9] and out["status"] == -77 and (out["backup"] == 6.0).all() and out["cost"] == 3.0


def scripted(phases, n_pairs=3, **kw):
    """Pairs on static records: a phase with conv_tol = 0 takes max_iters launches, one with conv_tol > 0 two (a step, then converged)."""
    rng = np.random.default_rng(7)
    recs = [ref.make_records(rng, 2, 3, 2, residual_scale=0.25) for _ in range(n_pairs)]
    sched = sv.sched_info(phases, **kw)
    states = [sv.with_verdict_state(ref.new_state(np.eye(4), np.ones(2), 5, lam0=1.0, scheduled=True)) for _ in range(n_pairs)]
    for s in states:
        s["phase"] = sched["entry"]
    v = sv.Verdict(retry_mask=sv.LAST_CAP)
    step = lambda i, s, idle: sv.schedule_step_ref(lambda p: recs[i], s, sched, v, np.ones(2, f32), np.eye(4, dtype=f32).ravel(), idle_mask=idle)
    return states, step, sched, v


def test_run_ref_round_counts():
    phases = [dict(max_iters=3), dict(max_iters=9, conv_tol=0.5), dict(max_iters=4)]          # 3 + 2 + 4 launches
    states, step, sched, v = scripted(phases)
    rounds, poll, out = sv.run_ref(states, step, sched, v, 4, 100)
    assert rounds == 12 and poll == [3, 0, 0, 0, 0] and all(s["status"] == sv.LAST_CAP and s["evals"][:3].tolist() == [3, 2, 4] for s in out)
    assert sv.run_ref(states, step, sched, v, 3, 100)[0] == 9 and sv.run_ref(states, step, sched, v, 1, 100)[0] == 9
    rounds, poll, out = sv.run_ref(states, step, sched, v, 4, 7)                               # cut in the last phase
    assert rounds == 7 and poll == [2, 0, 0, 3, 0b100] and all(s["status"] == sv.UNFINISHED and (s["phase"], s["iters"]) == (2, 2) for s in out)


def test_run_ref_a_restart_into_an_adam_phase_sits_out_until_the_next_poll():
    phases = [dict(max_iters=3, flags=sv.PHASE_ADAM, next=2), dict(max_iters=5)]
    states, step, sched, v = scripted(phases, entry=1, retry2_entry=0)
    # launches 1..5 the first attempt (poll at 4: only phase 1 is occupied), restart at 5; 6, 7, 8 sat out; poll at 8 sees phase 0; 9, 10, 11 Adam
    rounds, poll, out = sv.run_ref(states, step, sched, v, 4, 100)
    assert rounds == 12 and poll == [2, 0, 0, 0, 0]
    assert all(s["status"] == sv.LAST_CAP | sv.RETRIED | sv.ADAM and s["evals"][:2].tolist() == [3, 5] and s["attempts"] == 2 for s in out)
    assert sv.run_ref(states, step, sched, v, 1, 100)[0] == 8                                  # polled every round nobody waits
    rounds, poll, _ = sv.run_ref(states, step, sched, v, 4, 4)
    assert rounds == 4 and poll == [1, 0, 1, 3, 0b10]                                          # an attempt is left
