"""-m gpu: everything k_pairs_gn_sched (csrc/sp_solver.hip) does AFTER the per-pair solve -- the verdict (SpVerdict), the retry decision,
the in-place restart of a second and third attempt, the SpQueue slot refill -- and k_phase_min, k_mark_unfinished and the host loop
schedule_run, against tests/schedule_verdict_ref.py (numpy, written from include/sp_hip.h) on top of the float64 solve of gn_step_ref.py.

The rig is test_gpu_gn_step.py's (tests/gn_step_rig.py): hand-made partial records, three pairs per launch, the middle one under test,
every buffer a call may write compared (the neighbours, the unused kld tails and a sentinel entry in front of and behind the pairs'
status / diag / attempts / evals included), the reference continuing from the device's values after each call.  A run launches no cost
pass for a phase with n_spans = 0 (a queue run: max_spans = 0), so sp_pairs_schedule_run[_queue] are driven from static records too.

The usual case (``finish``): one phase {max_iters 5, conv_tol 0.75}; call 1 steps at cost 4, then the test rounds the log-depths to
multiples of 1/64, sets kld0 / pose0, the segment columns [8] / [9] and the thresholds; call 2 converges at cost 3 (no step) and files
the verdict -- every tested quantity is then an exactly representable number the test chose.

Bounds.  Decisions, integers, status, diag[1, 3, 4, 6, 7] bitwise; diag[0, 2, 5] by test_gpu_gn_step's cost rule (bitwise on dyadic
records); pose / kld of a stepped call within 2 ulp; run-level comparisons are device against device: bitwise.  Thresholds are moved by
2^-9 of themselves (the library is compiled with -ffp-contract=on; nothing here is decided closer than 1e-3), ties are exact.

PINNED AS IT IS TODAY (the header now says so): pose entries 12..15 are not tested for finiteness; a magnitude above 3e38 counts as
non-finite; diag[7] is reported also when fewer than 8 segments are judged (diag[6] = 0); lm_state[5, 6] survive a restart; a first cost of
exactly 0 is not captured (the next evaluation's is).

Case -> branch
  test_each_bit_alone                 kld_bound / cost_bound / cost_ratio (against the captured diag[5]) / valid_min / the three segment rules:
                                      just above, just below, an exact tie (not flagged), the bound <= 0 (off)
  test_last_cap                       lm_state[7] > 0: the last phase left on its cap / by its convergence test
  test_nonfinite_log_depth            NaN, +inf in kld[n], n across the 256-thread stride and all four waves; dmax over the finite entries only
  test_nonfinite_pose_and_cost        inf in pose entries 0 and 11; entry 12 (not looked at); a NaN cost
  test_reductions                     the largest excursion and the largest segment cost in each wave in turn, N = 1, 5, 12, 300
  test_segment_floors                 7 / 8 judged segments, 63 / 64 valid points, segments without records, equal costs (tie-break by index)
  test_segment_cap                    N = 2050: an outlier at segment 2047 (judged) and at 2048 (not looked at)
  test_first_cost_of_zero             the diag[5] capture when the first cost is exactly 0
  test_attempts                       retry_entry only / retry2_entry only / both / a failing bit outside retry_mask / attempts == NULL; after each
                                      restart the whole reset state
  test_restart_zeroes_one_slots_adam_moments   the Adam moments of the restarted slot only
  test_check_schedule_einval          check_schedule
  test_evals                          SpVerdict.evals per pair and phase over a scripted walk (with and without a verdict)
  test_run_matches_call_by_call       sp_pairs_schedule_run against the same schedule call by call, rounds and flag_host[0..4] against run_ref:
                                      a run that finishes, one cut by max_rounds, one with a third attempt in SP_PHASE_ADAM phases (sit-out rounds)
  test_run_257_pairs                  k_phase_min's stride loop, k_mark_unfinished's second block
  test_queue                          sp_pairs_schedule_run_queue: 3 pairs through 1 and 2 slots, 9 pairs through 8 slots with a 40-iteration
                                      tail over the `active` list; every pair bitwise the all-resident run
"""
import numpy as np
import pytest
import torch

import gn_step_ref as ref
import schedule_verdict_ref as sv
from gn_step_ref import f32
from gn_step_rig import DIAG_SENTINEL, STATUS_SENTINEL, Rig, make_pair, neighbours, set_cost, set_segment_cost
from gpu_util import T, npy

pytestmark = pytest.mark.gpu

UP, DOWN = 1 + 2.0 ** -9, 1 - 2.0 ** -9
C1, C2 = 4.0, 3.0                                    # the cost of the first call (captured in diag[5]) and of the one that converges
RPS12 = [1, 4, 2, 9, 3, 2, 1, 8, 2, 2, 5, 1]
BASE = [1, 1, 2, 2, 2, 2, 3, 3, 4, 4, 4, 16]         # mean |r| of the 12 segments: median (rank 5) 2, maximum 16
ONE_PHASE = [dict(max_iters=5, conv_tol=0.75)]
EINVAL = -1                                          # SP_EINVAL


def rps_for(N):
    return RPS12 if N == 12 else 2


def with_segment_costs(rec, costs, points=64.0):
    """A copy of ``rec`` whose segment n has mean |r| = costs[n] over ``points`` valid points (a segment without records is left alone)."""
    out = dict(rec, seg=rec["seg"].copy())
    sto = rec["pair"]["seg_tile_off"]
    pts = np.broadcast_to(points, (len(costs),))
    for n, c in enumerate(costs):
        if sto[n + 1] > sto[n]:
            set_segment_cost(out, n, 3.0 * pts[n] * c, pts[n])
    return out


def settle(rig, i, excursions):
    """Pair i's log-depths rounded to multiples of 1/64 (device and reference) and kld0 = kld - excursions."""
    N = rig.Ns[i]
    kld = (np.round(npy(rig.kld)[i, :N].astype(np.float64) * 64) / 64).astype(f32)
    rig.kld[i, :N] = T(kld)
    rig.ref[i]["kld"] = kld.copy()
    rig.kld0[i, :N] = T((kld - np.asarray(excursions, f32)).astype(f32))
    torch.cuda.synchronize()


def finish(pairs, v, second=None, excursions=None, phases=ONE_PHASE, c2=C2, between=None, what="", **rig_kw):
    """Call 1 steps at cost C1; then ``second`` (the middle pair's records of call 2), the excursions and ``between(rig)``; call 2 at cost
    c2 takes the pairs out of their only phase.  Returns (rig, the reference's info of the middle pair's last call)."""
    rig = Rig(pairs, entry="sched", phases=phases, verdict=v, **rig_kw)
    recs = [p["rec"] for p in pairs]
    rig.load([set_cost(r, C1) for r in recs])
    assert rig.step(what=f"{what} call 1")[1]["decision"] == "step"
    settle(rig, 1, np.full(rig.Ns[1], 0.125) if excursions is None else excursions)
    recs2 = [recs[0], second if second is not None else recs[1], recs[2]]
    rig.load([r if c2 is None else set_cost(r, c2) for r in recs2])
    if between:
        between(rig)
    info = rig.step(what=f"{what} call 2")[1]
    return rig, info


def mid12(rng):
    a, b = neighbours(rng)
    return [a, make_pair(rng, 12, RPS12, 6), b]


def filed(rig, i=1):
    return int(npy(rig.status)[i + 1]), npy(rig.diag)[i + 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# each bit alone
# ---------------------------------------------------------------------------------------------------------------------------------
# (verdict field, the value the tested quantity ties the bound at, the bit, the sense of the test); the quantities: cost 3, first cost 4,
# excursion 1/4, segment costs BASE (median 2, maximum 16), valid fraction n_rows / P (None: taken from the records)
THRESHOLDS = [("kld_bound", 0.25, sv.DEPTH_RANGE, ">"), ("cost_bound", 3.0, sv.COST, ">"), ("cost_ratio", 0.75, sv.COST, ">"), ("valid_min", None, sv.VALID, "<"),
              ("seg_max_ratio", 8.0, sv.SEGMENTS, ">"), ("seg_mean_ratio", 1.5, sv.SEGMENTS, ">"), ("seg_product", 4.0, sv.SEGMENTS, ">")]


@pytest.mark.parametrize("case", ["above", "below", "tie", "off"])
@pytest.mark.parametrize("field,tie,bit,sense", THRESHOLDS, ids=[t[0] for t in THRESHOLDS])
def test_each_bit_alone(field, tie, bit, sense, case):
    rng = np.random.default_rng(6000)
    pairs = mid12(rng)
    rec = pairs[1]["rec"]
    if tie is None:
        tie = float(f32(rec["span"][:, 28].astype(np.float64).sum() / rec["pair"]["P"]))
    flagged, clear = (tie * DOWN, tie * UP) if sense == ">" else (tie * UP, tie * DOWN)
    bound = dict(above=flagged, below=clear, tie=tie, off=0.0)[case]
    if sense == "<":
        bound = dict(above=clear, below=flagged, tie=tie, off=0.0)[case]           # "above" / "below" name the QUANTITY's side of the bound
    exc = np.full(12, 0.125)
    exc[7] = 0.25
    rig, info = finish(pairs, sv.Verdict(**{field: float(f32(bound))}), with_segment_costs(rec, BASE), exc, what=f"{field} {case}")
    assert info["decision"] == "converged" and npy(rig.phase)[1] == 1
    status, diag = filed(rig)
    fires = (case == "above") if sense == ">" else (case == "below")
    assert status == (bit if fires else 0), f"{field} = {bound!r} ({case}): status {status:#x}"
    assert diag.tolist() == [C2, 0.25, f32(rec["span"][:, 28].sum() / rec["pair"]["P"]), 1.0, 1.0, C1, 2.0, 16.0]


@pytest.mark.parametrize("how", ["cap", "converged"])
def test_last_cap(how):
    rng = np.random.default_rng(6100)
    phases = [dict(max_iters=2, conv_tol=0.75)]
    rig, info = finish(mid12(rng), sv.Verdict(), phases=phases, c2=0.5 if how == "cap" else C2, what=f"last phase left: {how}")
    assert info["decision"] == ("step" if how == "cap" else "converged")
    status, diag = filed(rig)
    assert status == (sv.LAST_CAP if how == "cap" else 0) and diag[3] == (2.0 if how == "cap" else 1.0) and npy(rig.lm_state)[1, 7] == (2 if how == "cap" else -1)


# ---------------------------------------------------------------------------------------------------------------------------------
# NONFINITE
# ---------------------------------------------------------------------------------------------------------------------------------
def mid300(rng, N=300):
    a, b = neighbours(rng)
    return [a, make_pair(rng, N, rps_for(N), 6), b]


@pytest.mark.parametrize("bad", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("n", [0, 255, 256, 299])
def test_nonfinite_log_depth(n, bad):
    rng = np.random.default_rng(6200)
    exc = np.full(300, 0.125)
    exc[(n + 100) % 300] = 0.375                     # the largest finite excursion sits elsewhere

    def between(rig):
        rig.poke(1, kld={n: bad})
    rig, info = finish(mid300(rng), sv.Verdict(kld_bound=1.0), excursions=exc, between=between, what=f"kld[{n}] = {bad}")
    status, diag = filed(rig)
    assert status == sv.NONFINITE and diag[1] == 0.375, "dmax is the maximum over the finite entries"
    got = npy(rig.kld)[1, n]
    assert np.isnan(got) if np.isnan(bad) else got == bad
    assert [filed(rig, i)[0] for i in (0, 2)] == [0, 0]


@pytest.mark.parametrize("what", ["pose0", "pose11", "pose12", "cost"])
def test_nonfinite_pose_and_cost(what):
    rng = np.random.default_rng(6300)
    pairs = mid12(rng)
    if what == "cost":
        nan_cost = set_cost(pairs[1]["rec"], C2)
        nan_cost["span"][0, 0] = np.nan
        rig, info = finish(pairs, sv.Verdict(cost_bound=1.0, cost_ratio=0.5), phases=[dict(max_iters=2, conv_tol=0.75)], c2=None, second=nan_cost, what="NaN cost")
        status, diag = filed(rig)             # a NaN cost neither converges nor is rejected: the call steps and leaves on the cap; no comparison holds
        assert status == sv.NONFINITE | sv.LAST_CAP and np.isnan(diag[0]) and np.isnan(npy(rig.costs)[1]) and diag[5] == C1
        return
    k = int(what[4:])
    rig, info = finish(pairs, sv.Verdict(), between=lambda rig: rig.poke(1, pose={k: np.inf}), what=what)
    status, diag = filed(rig)
    assert status == (sv.NONFINITE if k < 12 else 0), "pose entries 0..11 are tested, the last row is not (pinned)"
    assert npy(rig.pose)[1, k] == np.inf and diag[1] == 0.125


# ---------------------------------------------------------------------------------------------------------------------------------
# the two reductions over the workgroup
# ---------------------------------------------------------------------------------------------------------------------------------
PLACES = [(1, 0), (5, 0), (5, 4), (12, 0), (12, 11), (300, 3), (300, 70), (300, 130), (300, 200), (300, 255), (300, 290)]


@pytest.mark.parametrize("N,at", PLACES)
def test_reductions(N, at):
    """The largest excursion and the largest segment cost at segment ``at``: thread at % 256, wave (at % 256) / 64."""
    rng = np.random.default_rng(6400 + N)
    a, b = neighbours(rng)
    mid = make_pair(rng, N, rps_for(N), 6)
    exc, costs = np.full(N, 0.125), 1.0 + (np.arange(N) % 5) / 4.0
    exc[at], costs[at] = 0.5, 40.0
    v = sv.Verdict(kld_bound=0.25, seg_max_ratio=8.0)
    rig, info = finish([a, mid, b], v, with_segment_costs(mid["rec"], costs), exc, what=f"N={N} largest at {at}")
    status, diag = filed(rig)
    assert diag[1] == 0.5 and diag[7] == 40.0 and diag[6] == (0.0 if N < 8 else np.sort(costs)[(N - 1) // 2])
    assert status == sv.DEPTH_RANGE | (sv.SEGMENTS if N >= 8 else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the within-pair segment test
# ---------------------------------------------------------------------------------------------------------------------------------
SEGMENT_CASES = {
    #                 (records per segment, segment costs, valid points per segment) -> (diag[6], diag[7], SEGMENTS flagged at seg_max_ratio = 4)
    "8 judged": (RPS12, BASE, [64] * 8 + [63] * 4, (2.0, 3.0, False)),                       # 1 1 2 2 2 2 3 3: rank 3
    "7 judged": (RPS12, BASE, [64] * 7 + [63] * 5, (0.0, 3.0, False)),
    "outlier with 64 points": (RPS12, BASE, [64] * 12, (2.0, 16.0, True)),
    "outlier with 63 points": (RPS12, BASE, [64] * 11 + [63], (2.0, 4.0, False)),          # 11 judged: rank 5
    "more points": (RPS12, BASE, [64, 65, 128, 96, 4096, 64, 80, 64, 72, 64, 64, 1024], (2.0, 16.0, True)),
    "no records": ([1, 4, 0, 9, 3, 0, 1, 8, 2, 2, 5, 1], BASE, [64] * 12, (3.0, 16.0, True)),     # 10 judged: rank 4 of 1 1 2 2 3 3 4 4 4 16
    "all equal": (RPS12, [2] * 12, [64] * 12, (2.0, 2.0, False)),
    "two values": (RPS12, [1, 3] * 6, [64] * 12, (1.0, 3.0, False)),                        # rank 5 of 1 1 1 1 1 1 3 3 3 3 3 3
    "ties around the median": (RPS12, [3, 2, 2, 1, 2, 2, 3, 1, 2, 3, 9, 2], [64] * 12, (2.0, 9.0, True)),
}


@pytest.mark.parametrize("name", list(SEGMENT_CASES))
def test_segment_floors(name):
    rps, costs, points, (med, mx, flagged) = SEGMENT_CASES[name]
    rng = np.random.default_rng(6500)
    a, b = neighbours(rng)
    mid = make_pair(rng, 12, rps, 6)
    rig, info = finish([a, mid, b], sv.Verdict(seg_max_ratio=4.0), with_segment_costs(mid["rec"], costs, np.array(points, np.float64)), what=name)
    status, diag = filed(rig)
    assert (diag[6], diag[7]) == (med, mx) and status == (sv.SEGMENTS if flagged else 0), (name, diag[6], diag[7], status)


@pytest.mark.parametrize("at", [2047, 2048])
def test_segment_cap(at):
    """N = 2050: the first 2048 segments are looked at.  One call: the only phase has max_iters = 1, the verdict follows the step."""
    rng = np.random.default_rng(6600)
    a, b = neighbours(rng)
    mid = make_pair(rng, 2050, 1, 4)
    costs = 1.0 + (np.arange(2050) % 4) / 4.0             # 512 each of 1, 1.25, 1.5, 1.75 among the first 2048: rank 1023 is 1.25
    costs[at] = 64.0
    mid["rec"] = set_cost(with_segment_costs(mid["rec"], costs), C2)
    rig = Rig([a, mid, b], entry="sched", phases=[dict(max_iters=1)], verdict=sv.Verdict(seg_max_ratio=8.0))
    info = rig.step(what=f"N=2050 outlier at {at}")[1]
    status, diag = filed(rig)
    assert info["decision"] == "step" and diag[6] == 1.25 and diag[7] == (64.0 if at == 2047 else 1.75)
    assert status == sv.LAST_CAP | (sv.SEGMENTS if at == 2047 else 0)


def test_first_cost_of_zero():
    """PINNED: diag[5] takes the first evaluated cost that is not exactly 0 -- a first cost of 0 leaves it for the next evaluation."""
    rng = np.random.default_rng(6700)
    pairs = mid12(rng)
    rig = Rig(pairs, entry="sched", phases=[dict(max_iters=3)], verdict=sv.Verdict(cost_ratio=0.5))
    for k, cost in enumerate([0.0, 0.0, 0.5]):
        rig.load([set_cost(p["rec"], cost if i == 1 else C1) for i, p in enumerate(pairs)])
        rig.step(what=f"zero cost call {k}")
        assert npy(rig.diag)[2, 5] == cost and npy(rig.diag)[1, 5] == C1
    # the middle pair: 0.5 > 0.5 x 0.5, the cost of the third call counted as its first; the neighbour: 4 > 0.5 x 4
    assert filed(rig)[0] == sv.LAST_CAP | sv.COST and filed(rig, 0)[0] == sv.LAST_CAP | sv.COST


# ---------------------------------------------------------------------------------------------------------------------------------
# attempts
# ---------------------------------------------------------------------------------------------------------------------------------
# phases {R2, R1, E}, each one iteration and then out of the schedule: an attempt is ONE call, and every attempt fails kld_bound = 1e-6
ATTEMPT_PHASES = [dict(max_iters=1, next=3), dict(max_iters=1, next=3), dict(max_iters=1)]
ATTEMPTS = {
    #                       retry_entry, retry2_entry, retry_mask, attempts array -> the phases the pair visits, attempts, status bits on top, diag[4]
    "retry_entry only": (1, -1, sv.DEPTH_RANGE, True, [2, 1], 1, sv.RETRIED, 2),
    "retry2_entry only": (-1, 0, sv.DEPTH_RANGE, True, [2, 0], 2, sv.RETRIED | sv.ADAM, 3),
    "both": (1, 0, sv.DEPTH_RANGE, True, [2, 1, 0], 2, sv.RETRIED | sv.ADAM, 3),
    "outside retry_mask": (1, 0, sv.COST | sv.VALID | sv.SEGMENTS | sv.NONFINITE, True, [2], 0, 0, 1),
    "attempts NULL": (1, 0, 0, False, [2], None, 0, 1),
    "no retry entries": (-1, -1, sv.DEPTH_RANGE, True, [2], 0, 0, 1),
}


@pytest.mark.parametrize("name", list(ATTEMPTS))
def test_attempts(name):
    r1, r2, mask, counted, visits, attempts, extra, made = ATTEMPTS[name]
    rng = np.random.default_rng(6800)
    pairs = mid12(rng)
    for p in pairs:
        p["phase"] = 2
    rig = Rig(pairs, entry="sched", phases=ATTEMPT_PHASES, verdict=sv.Verdict(kld_bound=1e-6, retry_mask=mask, lam0=0.125), attempts=counted,
              sched_entry=2, retry_entry=r1, retry2_entry=r2, evals=True)
    kld0, pose0, lam = npy(rig.kld).copy(), npy(rig.pose).copy(), [p["lam0"] for p in pairs]
    for k, ph in enumerate(visits):
        assert npy(rig.phase).tolist() == [ph] * 3
        rig.load([set_cost(p["rec"], C1 / (k + 1)) for p in pairs])
        infos = rig.step(what=f"{name}: attempt {k + 1}")
        assert all(i["decision"] == "step" and i["verdict"]["bits"] == sv.DEPTH_RANGE | sv.LAST_CAP for i in infos)
        lm, last = npy(rig.lm_state), k == len(visits) - 1
        if not last:             # restarted in that launch (Rig.step has compared every buffer with restart_ref's; the headlines again, by hand)
            assert all(i["verdict"]["again"] == (1 if visits[k + 1] == 1 else 2) for i in infos)
            assert np.array_equal(npy(rig.kld).view(np.uint32), kld0.view(np.uint32)) and np.array_equal(npy(rig.pose).view(np.uint32), pose0.view(np.uint32))
            assert npy(rig.status).tolist() == [STATUS_SENTINEL] * 5 and (npy(rig.diag)[1:4, [0, 1, 2, 3, 4, 6, 7]] == DIAG_SENTINEL).all()
            assert (npy(rig.diag)[1:4, 5] == 0).all() and npy(rig.iters).tolist() == [0, 0, 0] and not npy(rig.adam_state).any()
            for i in range(3):
                assert lm[i].tolist() == [0.125, -1.0, k + 1, 0, 0, f32(C1 / (k + 1)), lm[i, 6], 0] and lm[i, 6] > 0.9
        else:
            assert npy(rig.phase).tolist() == [3] * 3 and npy(rig.status)[1:4].tolist() == [sv.DEPTH_RANGE | sv.LAST_CAP | extra] * 3
            assert npy(rig.diag)[1:4, 4].tolist() == [made] * 3 and npy(rig.diag)[1:4, 5].tolist() == [f32(C1 / (k + 1))] * 3
            assert lm[:, 2].tolist() == [k + 1] * 3
    if counted:
        assert npy(rig.attempts)[1:4].tolist() == [attempts] * 3
    want_evals = np.zeros((3, sv.MAX_PHASES), np.int32)
    want_evals[:, visits] = 1
    assert np.array_equal(npy(rig.evals)[1:4], want_evals)
    infos = rig.step(what=f"{name}: finished")            # a finished pair is left alone
    assert [i["decision"] for i in infos] == ["finished"] * 3


def test_restart_zeroes_one_slots_adam_moments():
    """retry2_entry only, SP_PHASE_ADAM phases: the middle pair leaves the entry phase (one Adam iteration), fails and restarts at phase 0 with
    its moments zeroed; the neighbours, two iterations into phase 0, keep theirs."""
    from super_primitive_amd import _lib
    rng = np.random.default_rng(6900)
    pairs = mid12(rng)
    pairs[1]["phase"] = 1
    phases = [dict(max_iters=4, flags=_lib.SP_PHASE_ADAM, next=2), dict(max_iters=2, flags=_lib.SP_PHASE_ADAM)]
    rig = Rig(pairs, entry="sched", phases=phases, verdict=sv.Verdict(retry_mask=sv.LAST_CAP, lam0=0.125), sched_entry=1, retry2_entry=0)
    kld0 = npy(rig.kld).copy()
    for k in range(2):
        infos = rig.step(what=f"adam restart call {k}")
        assert [i["decision"] for i in infos] == ["adam"] * 3
    adam = npy(rig.adam_state)
    assert infos[1]["verdict"]["again"] == 2 and not adam[1].any() and adam[0, 0] == 2 and adam[2, 0] == 2 and adam[0, 2:].any() and adam[2, 2:].any()
    assert np.array_equal(npy(rig.kld)[1], kld0[1]) and npy(rig.attempts).tolist() == [7, 0, 2, 0, 7] and npy(rig.phase).tolist() == [0, 0, 0]
    infos = rig.step(what="adam restart call 2")          # the third attempt's first iteration starts from zero moments
    assert npy(rig.adam_state)[:, 0].tolist() == [3, 1, 3]


def test_check_schedule_einval():
    from super_primitive_amd import _lib
    rng = np.random.default_rng(7000)
    rig = Rig(mid12(rng), entry="sched", phases=ATTEMPT_PHASES, verdict=sv.Verdict(retry_mask=sv.COST), sched_entry=2, retry_entry=1, retry2_entry=0)

    def rc(edit_s=None, edit_v=None, verdict=True):
        s, v = rig.schedule(), rig.verdict_struct()
        if edit_s:
            edit_s(s)
        if edit_v:
            edit_v(v)
        return rig.call_sched_step(s, v if verdict else None)

    def field(name, value, phase=None):
        return lambda s: setattr(s if phase is None else s.phase[phase], name, value)

    before = rig.snapshot()
    bad_s = [field("n_phases", 0), field("n_phases", 13), field("entry", -1), field("entry", 3), field("retry_entry", -2), field("retry_entry", 3),
             field("retry2_entry", -2), field("retry2_entry", 3), field("max_iters", 0, 1), field("pairs", None, 0), field("span_partials", None, 2),
             field("seg_partials", None, 1), field("next", 1, 1), field("next", 4, 0), field("next", 2, 2)]
    for k, e in enumerate(bad_s):
        assert rc(e) == EINVAL, f"schedule edit {k}"

    def adam_without(what):
        def edit(s):
            s.phase[0].flags = _lib.SP_PHASE_ADAM
            setattr(s, what, 0)
        return edit
    for what in ("adam_state", "adam_lr_pose", "adam_lr_kld"):
        assert rc(adam_without(what)) == EINVAL, what
    for name in ("pose0", "kld0", "pose_base", "kld_base", "attempts"):
        assert rc(edit_v=lambda v, name=name: setattr(v, name, None)) == EINVAL, name
    torch.cuda.synchronize()
    after = rig.snapshot()
    assert all(np.array_equal(before[k], after[k], equal_nan=True) for k in before), "a refused call wrote something"
    # attempts == NULL is fine without a retry entry, or with retry_mask == 0
    ok = [dict(edit_s=lambda s: (setattr(s, "retry_entry", -1), setattr(s, "retry2_entry", -1)), edit_v=lambda v: setattr(v, "attempts", None)),
          dict(edit_v=lambda v: (setattr(v, "attempts", None), setattr(v, "retry_mask", 0))), dict(verdict=False)]
    for kw in ok:
        assert rc(**kw) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# evals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_verdict", [True, False])
def test_evals(with_verdict):
    rng = np.random.default_rng(7100)
    pairs = mid12(rng)
    pairs[0]["phase"], pairs[2]["phase"] = 1, 3            # one pair a phase ahead, one finished from the start
    phases = [dict(max_iters=2, next=2), dict(max_iters=3), dict(max_iters=9, conv_tol=0.5)]
    rig = Rig(pairs, entry="sched", phases=phases, verdict=sv.Verdict() if with_verdict else None, evals=True)
    for k in range(6):
        rig.step(what=f"evals call {k}")
    want = np.zeros((3, sv.MAX_PHASES), np.int32)
    want[0, 1:3], want[1, [0, 2]] = [3, 2], [2, 2]          # phase 2: a step, then converged
    assert np.array_equal(npy(rig.evals)[1:4], want) and npy(rig.phase).tolist() == [3, 3, 3]
    assert npy(rig.status)[1:4].tolist() == ([0, 0, STATUS_SENTINEL] if with_verdict else [STATUS_SENTINEL] * 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------------------------------------------------------------
def run_rig(kind, seed=7200):
    """The same three pairs, schedule and verdict every time it is called: per-phase record arrays, every phase with a system of its own."""
    from super_primitive_amd import _lib
    rng = np.random.default_rng(seed)
    pairs = mid12(rng)
    if kind == "third attempt":
        # {A (Adam, 3), R (4), E (5, the entry)}: every attempt ends on a cap and fails retry_mask = LAST_CAP
        phases = [dict(max_iters=3, flags=_lib.SP_PHASE_ADAM, next=3), dict(max_iters=4, next=3), dict(max_iters=5)]
        kw = dict(sched_entry=2, retry_entry=1, retry2_entry=0, verdict=sv.Verdict(retry_mask=sv.LAST_CAP, lam0=0.25))
    else:
        phases = [dict(max_iters=3), dict(max_iters=9, conv_tol=0.5, next=3), dict(max_iters=1), dict(max_iters=4)]
        kw = dict(verdict=sv.Verdict(kld_bound=1e-6, cost_bound=1.0))
    for p in pairs:
        p["phase"] = kw.get("sched_entry", 0)
    rig = Rig(pairs, entry="sched", phases=phases, evals=True, per_phase=True, **kw)
    shapes = [(5, [1, 0, 3, 2, 9], 3), (12, RPS12, 6), (9, 2, 70)]
    for k in range(len(phases)):
        rig.load([set_cost(ref.make_records(rng, *s, residual_scale=0.25), 2.0 ** -k) for s in shapes], phase=k)
    return rig


RUNS = {"finishes": ("plain", 4, 100, 12), "cut by max_rounds": ("plain", 4, 6, 6), "third attempt": ("third attempt", 4, 100, 16)}


@pytest.mark.parametrize("name", list(RUNS))
def test_run_matches_call_by_call(name):
    kind, check_every, max_rounds, rounds = RUNS[name]
    a, b = run_rig(kind), run_rig(kind)
    initial = [ref.copy_state(s) for s in b.ref]
    # call by call, every call pinned to the reference (no call sits out: a pair's result does not depend on when its launches happen)
    calls = 0
    while calls < max_rounds and (npy(a.phase) < len(a.phases)).any():
        a.step(what=f"{name} call {calls}")
        calls += 1
    got_rounds, flag = b.run(check_every, max_rounds)
    sa, sb = a.snapshot(), b.snapshot()
    if name == "cut by max_rounds":
        unfinished = sa["phase"] < len(a.phases)
        assert unfinished.all() and (sa["status"][1:4] == STATUS_SENTINEL).all()
        sa["status"][1:4] = sv.UNFINISHED
    else:
        assert (sa["phase"] == len(a.phases)).all()
    for k in sa:
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), f"{name}: {k} differs between the run and the same calls one by one"
    # the host loop: rounds and the poll record against run_ref (a pure simulation from the initial states)
    k0, p0 = npy(b.kld0), npy(b.pose0)
    step = lambda i, s, idle: sv.schedule_step_ref(b.recs_of(i), s, b.sched_info(), b.v, k0[i], p0[i], b.lm, b.adam_lr, idle_mask=idle)
    want_rounds, poll, states = sv.run_ref(initial, step, b.sched_info(), b.v, check_every, max_rounds)
    assert want_rounds == rounds, "the scripted schedule is not what the test means to run"
    assert got_rounds == want_rounds and flag[:5].tolist() == poll, (got_rounds, flag.tolist(), want_rounds, poll)
    assert [s["status"] for s in states] == sb["status"][1:4].tolist() and np.array_equal(np.stack([s["evals"] for s in states]), sb["evals"][1:4])
    if kind == "third attempt":
        assert sb["attempts"][1:4].tolist() == [2, 2, 2] and (sb["status"][1:4] == sv.LAST_CAP | sv.RETRIED | sv.ADAM).all()
        # the rounds a restarted pair sat out show in the count: polled every round, the same schedule takes 5 + 4 + 3 launches
        assert sv.run_ref(initial, step, b.sched_info(), b.v, 1, max_rounds)[0] == 12 < rounds


def test_run_257_pairs():
    """257 pairs of one segment, cut by max_rounds = 3: pairs that start in phase 1 finish (3 iterations), those in phase 0 do not, those in
    phase 2 were finished from the start.  Pair 256 starts in phase 0."""
    rng = np.random.default_rng(7300)
    phases = [dict(max_iters=2), dict(max_iters=3)]
    pairs = []
    for i in range(257):
        p = make_pair(rng, 1, 3, 1, lam0=1.0, phase=(i + 2) % 3)
        p["rec"] = set_cost(p["rec"], 1.0 + i / 256.0)
        pairs.append(p)
    rig = Rig(pairs, entry="sched", phases=phases, verdict=sv.Verdict(cost_bound=1.5), evals=True)
    initial = [ref.copy_state(s) for s in rig.ref]
    rounds, flag = rig.run(2, 3)
    k0, p0 = npy(rig.kld0), npy(rig.pose0)
    step = lambda i, s, idle: sv.schedule_step_ref(rig.recs_of(i), s, rig.sched_info(), rig.v, k0[i], p0[i], rig.lm, rig.adam_lr, idle_mask=idle)
    want_rounds, poll, states = sv.run_ref(initial, step, rig.sched_info(), rig.v, 2, 3)
    start = np.array([p["phase"] for p in pairs])
    assert rounds == want_rounds == 3 and poll == [1, 0, 0, int((start == 0).sum()), 0b10] and flag[:5].tolist() == poll
    status, s = npy(rig.status), rig.snapshot()
    assert status[0] == status[-1] == STATUS_SENTINEL
    assert (status[1:-1][start == 0] == sv.UNFINISHED).all() and (status[1:-1][start == 2] == STATUS_SENTINEL).all() and status[257] == sv.UNFINISHED
    want_done = np.array([sv.LAST_CAP | (sv.COST if 1.0 + i / 256.0 > 1.5 else 0) for i in range(257)])
    assert np.array_equal(status[1:-1][start == 1], want_done[start == 1])
    assert status[1:-1].tolist() == [st["status"] for st in states]
    assert s["phase"].tolist() == [st["phase"] for st in states] and s["iters"].tolist() == [st["iters"] for st in states]
    assert np.array_equal(s["evals"][1:-1], np.stack([st["evals"] for st in states]))
    assert np.array_equal(s["diag"][1:-1][:, [3, 4]], np.stack([st["diag"][[3, 4]] for st in states]))
    assert np.array_equal(s["diag"][1:-1][:, [0, 5]], np.stack([st["diag"][[0, 5]] for st in states]))           # dyadic costs: bitwise
    assert np.array_equal(s["lm_state"][:, [2, 3, 7]], np.stack([st["lm_state"][[2, 3, 7]] for st in states]))


def queue_rig(n_pairs):
    """Pairs of mixed layouts, all starting at lambda 0.5 (a queue gives every pair the same lam0).  Phases {R (40 iterations, conv_tol = 0),
    E (the entry)}: the LAST pair alone costs more than cost_bound, fails and restarts in R."""
    rng = np.random.default_rng(7400)
    shapes = [(5, [1, 0, 3, 2, 9], 3), (12, RPS12, 6), (9, 2, 70)]
    pairs = [make_pair(rng, *shapes[i % 3], lam0=0.5, phase=1) for i in range(n_pairs)]
    for i, p in enumerate(pairs):
        p["rec"] = set_cost(p["rec"], 8.0 if i == n_pairs - 1 else 1.0)
    phases = [dict(max_iters=40, next=2), dict(max_iters=2 if n_pairs > 3 else 3)]
    return Rig(pairs, entry="sched", phases=phases, verdict=sv.Verdict(cost_bound=2.0, kld_bound=1e-6, retry_mask=sv.COST, lam0=0.5), evals=True,
               sched_entry=1, retry_entry=0)


@pytest.mark.parametrize("n_pairs,n_slots", [(3, 1), (3, 2), (9, 8)])
def test_queue(n_pairs, n_slots):
    res = queue_rig(n_pairs)
    rounds, flag = res.run(2, 200)
    want, last = res.snapshot(), n_pairs - 1
    assert flag[0] == 2 and want["attempts"][1:-1].tolist() == [0] * last + [1] and want["evals"][last + 1, :2].tolist() == [40, want["evals"][1, 1]]
    assert want["status"][last + 1] == sv.RETRIED | sv.LAST_CAP | sv.COST | sv.DEPTH_RANGE and (want["status"][1:last + 1] == sv.LAST_CAP | sv.DEPTH_RANGE).all()
    q = queue_rig(n_pairs)
    out = q.run_queue(n_slots, 2, 400, lam0=0.5)
    got = q.snapshot()
    for k in ("pose", "kld", "status", "diag", "attempts", "evals"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), f"{k}: a pair's result depends on the slot it ran in"
    assert np.array_equal(out["q_lm"].view(np.uint32), want["lm_state"].view(np.uint32)) and np.array_equal(out["q_costs"].view(np.uint32), want["costs"].view(np.uint32))
    # head: the slots' first pairs and one per refill -- every finished pair asks once, also when nobody waits
    assert out["head"] == n_slots + n_pairs and out["head"] >= n_pairs and out["rounds"] <= 400 and out["flag"][0] == 2 and out["flag"][1] == out["head"]
    assert len(set(out["slot_pair"])) == n_slots and all(0 <= p < n_pairs for p in out["slot_pair"]) and out["phase"] == [2] * n_slots
    if n_slots == 8:
        # the last rounds ran over the `active` list alone: one busy slot of eight, the queue empty (8 x 1 <= 8) -- the 40-iteration attempt outlasts everyone
        assert out["rounds"] >= 2 + 2 + 40
