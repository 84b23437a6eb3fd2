"""-m gpu: ONE call of the per-pair Gauss-Newton / LM solver (solve_gn / solve_adam_sched in csrc/sp_solve_device.h, through
sp_pairs_gn_step, sp_pairs_gn_step_conv and sp_pairs_schedule_gn_step) against the float64 dense solve of tests/gn_step_ref.py.

The solver reads only the partial records and a few SpPair fields, so the records are hand-made (no image, no table).  The rig (Rig,
make_pair, neighbours, swap_cost) lives in tests/gn_step_rig.py, shared with test_gpu_schedule_verdict.py.  Every case
launches THREE pairs; the middle one is the pair under test, so its tile0, rec0, backup / lm_state / adam_state strides are non-zero and
max_N > N; the neighbours are compared with the reference as well (a write into a neighbour is a mismatch), and so is every buffer a
call may write: kld (with the unused tail of each pair's slot), pose, lm_state[0..7], backup, costs, done or phase / iters, the Adam
moments.  After each compared call the reference continues from the DEVICE's values, so every call is judged from identical inputs.

Bounds (derived, not tuned).  The device solves in float64 and rounds once to float32; every system's dense damped matrix is asserted
to have a condition number <= 1e6, so both float64 solves are good to ~1e-9 relative, far below a float32 ulp.  Hence kld and pose within
2 ulp of the reference (one for the cast of delta, one for the add); lm_state[0,2,3,4,7], done, phase, iters exact; lm_state[1,5,6] and
costs bitwise where the record entries are dyadic (every float64 sum exact in any order), else within 1 ulp; a call that takes no step
(reject, converged, finished) bitwise everywhere.  Adam: |delta param| <= 1e-6 lr + 1 ulp per iteration (a handful of float32 roundings
on a step of size <= lr), moments to 1e-6 of their vector's scale.

Case -> branch
  test_reduction_shapes          reduce_columns: n_tiles across its 8-group stride (G = 8 groups) and 8-deep trip; segment_system: 0..17
                                 records per segment across its 8-deep trip; a segment without records
  test_segment_counts            N across the 8-lane Schur stride and SP_SEG_CACHE = 256: the recompute path in the Schur sum and the update
  test_pose_only                 SP_PHASE_POSE_ONLY
  test_depth_damp                SP_PHASE_DEPTH_DAMP(k), also in the recompute path
  test_clamp                     the +-0.5 trust region; backup = the point left
  test_frozen_segments           D = 0, D (1 + lambda) = 5e-13 <= 1e-12, no records
  test_failed_pivot              ldlt_solve<6> returns false
  test_accept_reject_accept      the LM state machine of sp_pairs_gn_step: reject / restore / lambda x lm_up / no lowering after a rejection
  test_converges_and_stays_done  sp_pairs_gn_step_conv: done, and the early return of a done pair
  test_schedule_bookkeeping      iters, leave_phase on the cap (accepted and rejected iteration), by convergence, SpPhase.next, a finished pair
  test_predicted_exit            SP_PHASE_PREDICTED_EXIT (the gain, also in the recompute path), not at lambda = 0.1, not with depth damping
  test_adam_phase                SP_PHASE_ADAM (solve_adam_sched), its cap
  test_retract_branches          se3_retract_left: the solved twist steered into the 2-term series, the 3-term series and the closed form, from
                                 the identity pose (every entry at 2 ulp of its own magnitude against tests/se3_ref.py) and from a general one
"""
import numpy as np
import pytest

import gn_step_ref as ref
from gn_step_ref import f32
from gn_step_rig import SENTINEL, Rig, make_pair, neighbours, swap_cost
from gpu_util import npy

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------------------------
# reduction shapes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tiles", [1, 7, 8, 9, 63, 64, 65, 130])
def test_reduction_shapes(n_tiles):
    rng = np.random.default_rng(100 + n_tiles)
    a, b = neighbours(rng)
    mid = make_pair(rng, 9, [0, 1, 4, 7, 8, 9, 17, 8, 1], n_tiles)          # dyadic entries: every sum exact, costs bitwise
    rig = Rig([a, mid, b])
    info = rig.step(exact=True, what=f"n_tiles={n_tiles}")[1]
    assert info["decision"] == "step" and info["lam"] == 1.0 and info["active"].tolist() == [False] + [True] * 8


# ---------------------------------------------------------------------------------------------------------------------------------
# segment counts
# ---------------------------------------------------------------------------------------------------------------------------------
def boost_tail(rec, first=256):
    """Segments >= first get twice the coupling and eight times the gradient: dropping or mis-damping them moves the pose step."""
    sto = rec["pair"]["seg_tile_off"]
    rec["seg"][sto[first]:, 0:6] *= 2
    rec["seg"][sto[first]:, 7] *= 8


def pose_step_without_tail(rec, lam, depth_damp=0.0, first=256):
    _, H, bp, _, h, D, bd = ref.sum_records(rec["span"], rec["seg"], rec["pair"])
    return ref.dense_step(H, bp, h[:first], D[:first], bd[:first], lam, depth_damp)[0]


@pytest.mark.parametrize("lam", [1e-4, 1.0, 100.0])
@pytest.mark.parametrize("N", [1, 5, 8, 9, 255, 256, 257, 300])
def test_segment_counts(N, lam):
    rng = np.random.default_rng(1000 + N)
    a, b = neighbours(rng, exact=False)
    mid = make_pair(rng, N, 2 if N > 9 else 3, 5, exact=False, lam0=float(f32(lam) * 2))
    if N > 256:
        boost_tail(mid["rec"])
    rig = Rig([a, mid, b])
    info = rig.step(exact=False, what=f"N={N} lambda={lam}")[1]
    assert info["decision"] == "step" and info["lam"] == float(f32(lam)) and info["active"].all() and info["pose_ok"]
    if N > 256:
        short = pose_step_without_tail(mid["rec"], info["lam"])
        assert np.abs(short - info["dxi"]).max() > 1e-3 * np.abs(info["dxi"]).max(), "the segments beyond the cache do not matter enough"


# ---------------------------------------------------------------------------------------------------------------------------------
# branches
# ---------------------------------------------------------------------------------------------------------------------------------
BIG = [12, 300]


def rps_for(N):
    return [1, 4, 2, 9, 3, 2, 1, 8, 2, 2, 5, 1] if N == 12 else 2


@pytest.mark.parametrize("N", BIG)
def test_pose_only(N):
    from super_primitive_amd import _lib
    rng = np.random.default_rng(2000 + N)
    a, b = neighbours(rng)
    mid = make_pair(rng, N, rps_for(N), 6)
    rig = Rig([a, mid, b], entry="sched", phases=[dict(max_iters=50, flags=_lib.SP_PHASE_POSE_ONLY), dict(max_iters=50)])
    before = npy(rig.kld).copy()
    info = rig.step(what=f"pose_only N={N}")[1]
    assert info["decision"] == "step" and not info["active"].any() and not info["dd"].any()
    assert np.array_equal(npy(rig.kld).view(np.uint32), before.view(np.uint32)), "a pose-only phase moved a log-depth"
    _, H, bp, *_ = ref.sum_records(mid["rec"]["span"], mid["rec"]["seg"], mid["rec"]["pair"])
    np.testing.assert_allclose(info["dxi"], np.linalg.solve(H + np.diag(np.diag(H)) + 1e-12 * np.eye(6), -bp), rtol=1e-9)     # lambda = 1


@pytest.mark.parametrize("k", [1, 8, 96], ids=lambda k: f"damp{k / 8:g}")
@pytest.mark.parametrize("N", BIG)
def test_depth_damp(N, k):
    from super_primitive_amd import _lib
    rng = np.random.default_rng(2100 + N)
    a, b = neighbours(rng)
    mid = make_pair(rng, N, rps_for(N), 6)
    if N > 256:
        boost_tail(mid["rec"])
    rig = Rig([a, mid, b], entry="sched", phases=[dict(max_iters=50, flags=k << _lib.SP_PHASE_DEPTH_DAMP_SHIFT), dict(max_iters=50)])
    info = rig.step(what=f"depth_damp={k / 8} N={N}")[1]
    assert info["decision"] == "step" and info["active"].all() and info["pose_ok"]
    _, H, bp, _, h, D, bd = ref.sum_records(mid["rec"]["span"], mid["rec"]["seg"], mid["rec"]["pair"])
    undamped = ref.dense_step(H, bp, h, D, bd, 1.0, 0.0)
    assert np.abs(undamped[0] - info["dxi"]).max() > 1e-3 * np.abs(info["dxi"]).max(), "the damping does not matter enough"
    if N > 256:                    # ... nor does it when only the segments beyond the cache lose it
        D2 = D.copy()
        D2[256:] *= 2.0 / (2.0 + k / 8)
        part = ref.dense_step(H, bp, h, D2, bd, 1.0, k / 8)
        assert np.abs(part[0] - info["dxi"]).max() > 1e-3 * np.abs(info["dxi"]).max()


def special_indices(N):
    return dict(up=[0, 7], down=[3], zero=[1], tiny=[4], empty=[2]) if N == 12 else \
        dict(up=[0, 7, 270], down=[3, 299], zero=[1, 260], tiny=[4, 280], empty=[2, 290])


@pytest.mark.parametrize("N", BIG)
def test_clamp(N):
    rng = np.random.default_rng(2200 + N)
    a, b = neighbours(rng)
    idx = special_indices(N)
    mid = make_pair(rng, N, rps_for(N), 6)
    for n in idx["up"]:
        ref.set_segment(mid["rec"], n, h=np.zeros(6), D=4.0, bd=-24.0)       # at lambda = 1 its own step is 24 / 8 = +3
    for n in idx["down"]:
        ref.set_segment(mid["rec"], n, h=np.zeros(6), D=2.0, bd=12.0)        # -3
    rig = Rig([a, mid, b])
    info = rig.step(what=f"clamp N={N}")[1]
    assert np.allclose(info["unclamped"][idx["up"]], 3.0) and np.allclose(info["unclamped"][idx["down"]], -3.0)
    kld = npy(rig.kld)[1, :N]
    assert np.array_equal(kld[idx["up"]], mid["kld"][idx["up"]] + f32(0.5)) and np.array_equal(kld[idx["down"]], mid["kld"][idx["down"]] - f32(0.5))
    backup = npy(rig.backup)[1]
    assert np.array_equal(backup[:16], mid["pose"].ravel()) and np.array_equal(backup[16:16 + N], mid["kld"])
    assert (backup[16 + N:] == SENTINEL).all()


@pytest.mark.parametrize("N", BIG)
def test_frozen_segments(N):
    rng = np.random.default_rng(2300 + N)
    a, b = neighbours(rng)
    idx = special_indices(N)
    rps = np.array(np.broadcast_to(rps_for(N), (N,)))
    rps[idx["empty"]] = 0
    mid = make_pair(rng, N, rps, 6)
    for n in idx["zero"]:
        ref.set_segment(mid["rec"], n, h=[3, -2, 1, 2, -1, 4], D=0.0, bd=5.0)
    for n in idx["tiny"]:
        ref.set_segment(mid["rec"], n, h=[3, -2, 1, 2, -1, 4], D=2.5e-13, bd=5.0)      # D (1 + lambda) = 5e-13
    rig = Rig([a, mid, b])
    info = rig.step(what=f"frozen N={N}")[1]
    frozen = sorted(idx["zero"] + idx["tiny"] + idx["empty"])
    assert np.flatnonzero(~info["active"]).tolist() == frozen and info["pose_ok"]
    kld = npy(rig.kld)[1, :N]
    assert np.array_equal(kld[frozen].view(np.uint32), mid["kld"][frozen].view(np.uint32)), "a frozen segment moved"
    assert (kld[info["active"]] != mid["kld"][info["active"]]).mean() > 0.9


@pytest.mark.parametrize("N", BIG)
def test_failed_pivot(N):
    """PINNED AS IT IS TODAY: when the pose block is not positive definite after the elimination, the pose stays where it is bit for bit,
    every depth still takes its own (clamped) Newton step, and the call counts as an accepted step."""
    rng = np.random.default_rng(2400 + N)
    a, b = neighbours(rng)
    mid = make_pair(rng, N, rps_for(N), 6)
    n_bad = 5 if N == 12 else 290
    ref.set_segment(mid["rec"], n_bad, h=[100.0 if N == 12 else 1000.0, 0, 0, 0, 0, 0], D=1.0, bd=0.25)
    rig = Rig([a, mid, b])
    info = rig.step(what=f"failed pivot N={N}")[1]
    assert not info["pose_ok"] and not info["dxi"].any()
    assert np.array_equal(npy(rig.pose)[1].view(np.uint32), mid["pose"].ravel().view(np.uint32)), "the pose moved"
    kld, lm = npy(rig.kld)[1, :N], npy(rig.lm_state)[1]
    assert kld[n_bad] == mid["kld"][n_bad] - f32(0.125) and (kld != mid["kld"]).mean() > 0.9            # the depths are stepped
    assert lm[2] == 1 and lm[3] == 0 and lm[4] == 0 and lm[1] == npy(rig.costs)[1] and lm[0] == 1.0


# ---------------------------------------------------------------------------------------------------------------------------------
# state machine
# ---------------------------------------------------------------------------------------------------------------------------------
def two_systems(rng, N, rps, n_spans, **kw):
    p = make_pair(rng, N, rps, n_spans, **kw)
    other = ref.make_records(rng, N, rps, n_spans, residual_scale=0.25)
    return p, [p["rec"], other]


def run_script(rig, systems, scripts, what):
    """Call k loads, for pair i, system k % 2 of that pair with the cost of its first system times scripts[i][k]."""
    for k in range(len(scripts[0])):
        rig.load([swap_cost(systems[i][k % 2], systems[i][0], scripts[i][k]) for i in range(rig.n)])
        yield rig.step(what=f"{what} call {k}")


def three_pairs_two_systems(rng, **kw):
    specs = [(5, [1, 0, 3, 2, 9], 3), (12, rps_for(12), 6), (9, 2, 70)]
    made = [two_systems(rng, *s, **kw) for s in specs]
    return [m[0] for m in made], [m[1] for m in made]


def test_accept_reject_accept():
    rng = np.random.default_rng(3000)
    pairs, systems = three_pairs_two_systems(rng, lam0=0.25)
    rig = Rig(pairs)
    #                 down  up(+25 %)  back   down            the neighbours run other scripts in the same launches
    scripts = [(1.0, 0.5, 0.25, 0.375), (1.0, 0.5, 0.625, 0.5), (1.0, 1.5, 1.0, 2.0)]
    before_reject = None
    for k, infos in enumerate(run_script(rig, systems, scripts, "LM")):
        assert tuple(i["decision"] for i in infos) == [("step", "step", "step"), ("step", "step", "reject"), ("step", "reject", "step"),
                                                  ("reject", "step", "reject")][k]
        lm = npy(rig.lm_state)[1]
        if k == 1:
            before_reject = (npy(rig.backup)[1].copy(), lm[0])
        if k == 2:            # restored bit for bit from the backup, lambda x lm_up, flagged
            assert np.array_equal(npy(rig.pose)[1], before_reject[0][:16]) and np.array_equal(npy(rig.kld)[1, :12], before_reject[0][16:28])
            assert lm[0] == before_reject[1] * 8 and lm[4] == 1 and lm[3] == 1 and lm[2] == 2
        if k == 3:            # accepted after the rejection: lambda not lowered
            assert lm[0] == before_reject[1] * 8 and lm[4] == 0 and lm[2] == 3 and infos[1]["lam"] == lm[0]


def test_converges_and_stays_done():
    rng = np.random.default_rng(3100)
    pairs, systems = three_pairs_two_systems(rng, lam0=0.25)
    rig = Rig(pairs, entry="conv", conv_tol=1e-2)
    small = 1 - 2.0 ** -10        # a tenth of conv_tol; 0.5 -> 0.484375 is three times conv_tol (all factors dyadic: exact sums)
    scripts = [(1.0, 0.5, 0.484375, 0.484375 * small), (1.0, 0.5, 0.5 * small, 7.0), (1.0, 1.5, 1.0, small)]
    moved = []
    for k, infos in enumerate(run_script(rig, systems, scripts, "conv")):
        assert tuple(i["decision"] for i in infos) == [("step", "step", "step"), ("step", "step", "reject"), ("step", "converged", "step"),
                                                  ("converged", "skip", "converged")][k]
        moved.append((npy(rig.kld)[1].copy(), npy(rig.pose)[1].copy(), npy(rig.lm_state)[1].copy(), npy(rig.costs)[1]))
    assert npy(rig.done).tolist() == [1, 1, 1]
    assert np.array_equal(moved[1][0], moved[2][0]) and np.array_equal(moved[1][1], moved[2][1])           # converged: parameters untouched
    assert all(np.array_equal(x, y) for x, y in zip(moved[2], moved[3]))                                    # done: the call is a no-op


def test_schedule_bookkeeping():
    rng = np.random.default_rng(3200)
    pairs, systems = three_pairs_two_systems(rng, lam0=0.25)
    pairs[2]["phase"] = 4                              # already finished: untouched
    phases = [dict(max_iters=2, conv_tol=1e-2, next=2), dict(max_iters=1), dict(max_iters=3, conv_tol=1e-2), dict(max_iters=1, next=4)]
    rig = Rig(pairs, entry="sched", phases=phases)
    small = 1 - 2.0 ** -10
    # pair 0: cap on a REJECTED iteration, then phase 2: step, converged, phase 3: cap at once
    # pair 1: cap on an ACCEPTED iteration (skipping phase 1), phase 2: step, converged (-1), phase 3: one step, finished
    scripts = [(1.0, 1.5, 1.0, small, 0.5), (1.0, 0.5, 0.5, 0.5 * small, 0.25), (1.0,) * 5]
    want = [([("step", 0, 1, 0), ("reject", 2, 0, 2), ("step", 2, 1, 2), ("converged", 3, 0, -1), ("step", 4, 0, 1)]),
            ([("step", 0, 1, 0), ("step", 2, 0, 2), ("step", 2, 1, 2), ("converged", 3, 0, -1), ("step", 4, 0, 1)]),
            ([("finished", 4, 0, 0)] * 5)]
    for k, infos in enumerate(run_script(rig, systems, scripts, "schedule")):
        phase, iters, lm = npy(rig.phase), npy(rig.iters), npy(rig.lm_state)
        for i in range(3):
            assert (infos[i]["decision"], phase[i], iters[i], lm[i, 7]) == want[i][k], f"call {k} pair {i}"
            if k and phase[i] != want[i][k - 1][1]:
                assert lm[i, 1] == -1 and lm[i, 4] == 0 and iters[i] == 0          # a new phase starts afresh
    assert np.array_equal(npy(rig.kld)[2, :9], pairs[2]["kld"]) and npy(rig.costs)[2] == SENTINEL
    assert npy(rig.lm_state)[2].tolist() == [0.25, -1, 0, 0, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------------------
# predicted exit
# ---------------------------------------------------------------------------------------------------------------------------------
def with_gain_ratio(pair, ratio, conv_tol, lam, depth_damp=0.0):
    """The pair with its sum |r| scaled so that the PREDICTED gain of the step, -b . delta / (3 P), is ratio x conv_tol x cost."""
    rec = pair["rec"]
    sr, H, bp, _, h, D, bd = ref.sum_records(rec["span"], rec["seg"], rec["pair"])
    dxi, dd, active, _ = ref.dense_step(H, bp, h, D, bd, float(f32(lam)), depth_damp)
    gain = -(bp @ dxi + bd[active] @ dd[active])
    assert gain > 0
    ref.scale_cost(rec, gain / (ratio * float(f32(conv_tol))) / sr)
    return pair


@pytest.mark.parametrize("N", BIG)
def test_predicted_exit(N):
    from super_primitive_amd import _lib
    rng = np.random.default_rng(4000 + N)
    tol = 1e-2
    mk = lambda lam: make_pair(rng, N, rps_for(N), 6, lam0=float(f32(lam) * 2))
    stays = with_gain_ratio(mk(1e-3), 2.0, tol, 1e-3)
    leaves = with_gain_ratio(mk(1e-3), 0.5, tol, 1e-3)
    heavy = with_gain_ratio(mk(0.1), 0.5, tol, 0.1)              # lambda = 0.1 > 1e-2: no predicted exit
    if N > 256:
        for p in (stays, leaves, heavy):
            boost_tail(p["rec"])
        stays, leaves, heavy = with_gain_ratio(stays, 2.0, tol, 1e-3), with_gain_ratio(leaves, 0.5, tol, 1e-3), with_gain_ratio(heavy, 0.5, tol, 0.1)
    rig = Rig([stays, leaves, heavy], entry="sched", phases=[dict(max_iters=9, conv_tol=tol, flags=_lib.SP_PHASE_PREDICTED_EXIT), dict(max_iters=9)])
    before = npy(rig.kld).copy()
    infos = rig.step(exact=False, what=f"predicted exit N={N}")
    assert [i["predicted"] for i in infos] == [False, True, False]
    assert npy(rig.phase).tolist() == [0, 1, 0] and npy(rig.iters).tolist() == [1, 0, 1] and npy(rig.lm_state)[:, 7].tolist() == [0, -1, 0]
    assert (npy(rig.kld)[:, :N] != before[:, :N]).any(1).all(), "the step is applied either way"
    for info, ratio in zip(infos[:2], (2.0, 0.5)):
        assert abs(info["gain"] / (float(f32(tol)) * info["cost"]) - ratio) < 1e-3 * ratio
    if N > 256:                     # the segments beyond the cache decide: without their share the pair that stays would leave
        rec, info = stays["rec"], infos[0]
        _, _, bp, _, _, _, bd = ref.sum_records(rec["span"], rec["seg"], rec["pair"])
        short = -(bp @ info["dxi"] + bd[:256] @ info["dd"][:256]) / (3.0 * rec["pair"]["P"])
        assert short < 0.9 * float(f32(tol)) * info["cost"]


@pytest.mark.parametrize("N", BIG)
def test_no_predicted_exit_under_depth_damping(N):
    from super_primitive_amd import _lib
    rng = np.random.default_rng(4100 + N)
    tol = 1e-2
    mid = with_gain_ratio(make_pair(rng, N, rps_for(N), 6, lam0=2e-3), 0.5, tol, 1e-3, depth_damp=0.125)
    a, b = neighbours(rng)
    flags = _lib.SP_PHASE_PREDICTED_EXIT | (1 << _lib.SP_PHASE_DEPTH_DAMP_SHIFT)
    rig = Rig([a, mid, b], entry="sched", phases=[dict(max_iters=9, conv_tol=tol, flags=flags), dict(max_iters=9)])
    infos = rig.step(exact=False, what=f"predicted exit, damped N={N}")
    assert not infos[1]["predicted"] and npy(rig.phase).tolist() == [0, 0, 0] and npy(rig.iters).tolist() == [1, 1, 1]


# ---------------------------------------------------------------------------------------------------------------------------------
# SP_PHASE_ADAM
# ---------------------------------------------------------------------------------------------------------------------------------
def test_adam_phase():
    from super_primitive_amd import _lib
    rng = np.random.default_rng(5000)
    pairs, systems = three_pairs_two_systems(rng)
    rig = Rig(pairs, entry="sched", phases=[dict(max_iters=3, flags=_lib.SP_PHASE_ADAM), dict(max_iters=9)])
    assert not npy(rig.adam_state).any()
    for k, infos in enumerate(run_script(rig, systems, [(1.0, 0.5, 0.75)] * 3, "adam")):
        assert [i["decision"] for i in infos] == ["adam"] * 3
        assert npy(rig.adam_state)[:, 0].tolist() == [k + 1] * 3
        assert npy(rig.phase).tolist() == ([0] * 3 if k < 2 else [1] * 3) and npy(rig.iters).tolist() == ([k + 1] * 3 if k < 2 else [0] * 3)
    lm = npy(rig.lm_state)
    assert lm[:, 7].tolist() == [3, 3, 3] and lm[:, 1].tolist() == [-1] * 3 and lm[:, 2].tolist() == [3] * 3 and lm[:, 0].tolist() == [2.0] * 3
    assert (npy(rig.backup) == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# se3_retract_left in each of its branches
# ---------------------------------------------------------------------------------------------------------------------------------
H_DIAG = np.array([4.0, 8.0, 16.0, 2.0, 4.0, 8.0])
DIAG_COLS = 1 + np.array([0, 6, 11, 15, 18, 20])          # H_pp's diagonal in the span record's row-major upper triangle


def steered_pair(rng, xi):
    """A pair whose pose-only step at lambda = 1 is the twist xi (float32 values) to ~1e-12 relative: the pose system is diagonal with
    dyadic entries and b_p = -(1 + lambda) H_pp xi, all of it in the first span record (every float64 sum exact)."""
    mid = make_pair(rng, 5, 2, 3)          # lam0 = 2: lambda = 1 at the first step
    span = mid["rec"]["span"]
    span[:, 1:28] = 0
    span[0, DIAG_COLS] = H_DIAG
    b = -2.0 * H_DIAG * np.asarray(xi, np.float64)
    assert np.array_equal(b.astype(f32).astype(np.float64), b)
    span[0, 22:28] = b
    return mid


def retract_branch(phi):
    t = float(np.dot(phi, phi))
    return 0 if t < 1e-12 else 1 if t < 1e-4 else 2


@pytest.mark.parametrize("start", ["identity", "general"])
def test_retract_branches(start):
    """The solved twist lands in each branch of se3_retract_left (theta^2 = 0 with tau != 0, either side of 1e-12, 1e-8, either side of 1e-4,
    0.3).  From the identity pose the new pose IS Exp(xi), so a wrong series coefficient is not hidden under a unit-size entry: every entry
    within PAIR_ULPS = 2 ulp of its OWN magnitude of se3_ref.retract (scipy's expm, no branch on theta); an exact zero exactly.  From a
    general pose: the file's bound (the rig's own comparison, and the same against se3_ref).  Neighbours and every other buffer as always."""
    import se3_ref
    from super_primitive_amd import _lib
    seen, worst = set(), 0.0
    for k, (name, xi) in enumerate(se3_ref.pair_step_twists()):
        rng = np.random.default_rng(6000 + k)
        a, b = neighbours(rng)
        rig = Rig([a, steered_pair(rng, xi), b], entry="sched", phases=[dict(max_iters=50, flags=_lib.SP_PHASE_POSE_ONLY), dict(max_iters=50)])
        if start == "identity":
            rig.poke(1, pose=dict(enumerate(np.eye(4, dtype=f32).ravel())))
        before = rig.ref[1]["pose"].astype(np.float64)
        info = rig.step(what=f"retract {name} from {start}")[1]
        assert info["decision"] == "step" and info["lam"] == 1.0 and not info["active"].any()
        np.testing.assert_allclose(info["dxi"], xi, rtol=1e-9, atol=0)
        assert retract_branch(info["dxi"][3:]) == retract_branch(xi[3:]) and (xi[:3] != 0).all()
        seen.add((retract_branch(xi[3:]), bool(xi[3:].any())))
        got = npy(rig.pose)[1].reshape(4, 4)
        want = se3_ref.retract(info["dxi"], before)
        assert got[3].tolist() == [0, 0, 0, 1]
        d = se3_ref.own_ulps(got[:3], want[:3]).max()
        worst = max(worst, d)
        assert d <= se3_ref.PAIR_ULPS, f"{name} from {start}: {d:.3g} ulp of the entry's own magnitude from Exp(xi) pose"
    assert seen == {(0, False), (0, True), (1, True), (2, True)}
    print(f"retract branches from {start}: at most {worst:.3g} ulp (own magnitude) from se3_ref.retract")
