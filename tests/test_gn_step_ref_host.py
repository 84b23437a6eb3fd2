"""The float64 yardstick of the per-pair Gauss-Newton / LM call (tests/gn_step_ref.py) checked against independent statements of the
same things, without a GPU: its step against a least-squares solve of the rows the records were made from, its SE(3) exponential
against the oracle's closed form, its LM state machine against a sequence written out by hand."""
import numpy as np
import pytest
import torch

import gn_step_ref as ref
from gn_step_ref import GnArgs, f32


@pytest.mark.parametrize("N,rps", [(1, 3), (5, [1, 4, 2, 7, 9]), (40, 2)])
def test_undamped_step_is_the_least_squares_solution_of_the_rows(N, rps):
    rng = np.random.default_rng(7 + N)
    rec = ref.make_records(rng, N, rps, n_spans=5, residual_scale=0.25)         # exact: the records ARE the rows' normal equations
    _, H, bp, _, h, D, bd = ref.sum_records(rec["span"], rec["seg"], rec["pair"])
    dxi, dd, active, info = ref.dense_step(H, bp, h, D, bd, lam=0.0)
    want_xi, want_d = ref.lstsq_step(rec["rows"], N)
    assert active.all() and info["pose_ok"] and info["cond"] <= 1e6
    assert np.abs(info["unclamped"]).max() < 0.5, "a clamp is active: choose a smaller residual_scale"
    scale = max(np.abs(want_xi).max(), np.abs(want_d).max())
    np.testing.assert_allclose(dxi, want_xi, rtol=1e-9, atol=1e-9 * scale)
    np.testing.assert_allclose(dd, want_d, rtol=1e-9, atol=1e-9 * scale)


@pytest.mark.parametrize("theta", [0.0, 1e-7, 1e-3, 0.3, 3.0])
def test_se3_exponential(theta):
    from oracle.photometric_oracle import se3_exp
    axis = np.array([2.0, -1.0, 2.0]) / 3.0
    xi = np.concatenate([[0.3, -0.2, 0.5], theta * axis])
    T = ref.se3_exp(xi)
    np.testing.assert_allclose(T @ ref.se3_exp(-xi), np.eye(4), rtol=0, atol=1e-14)
    np.testing.assert_allclose(T, se3_exp(torch.from_numpy(xi)).numpy(), rtol=0, atol=1e-14)
    np.testing.assert_allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), rtol=0, atol=1e-14)
    assert np.array_equal(T[3], [0, 0, 0, 1])


def test_retraction_by_zero_keeps_every_bit():
    pose = ref.random_pose(np.random.default_rng(3))
    assert np.array_equal(ref.retract(pose, np.zeros(6)).view(np.uint32), pose.view(np.uint32))


def _scripted(conv_tol, scheduled, max_iters=1 << 30):
    """cost: 1 -> 1/2 (down) -> 1/4 (down) -> 3/8 (up) -> 1/4 again at the restored point -> 1/4 (1 - 2^-10) (down by less than tol)."""
    rng = np.random.default_rng(11)
    base = ref.make_records(rng, 4, 2, n_spans=3, residual_scale=0.25)
    args = GnArgs(lm_up=8.0, lm_down=0.5, lm_min=1e-7, conv_tol=conv_tol, max_iters=max_iters, next_phase=3)
    st = ref.new_state(ref.random_pose(rng), 1.0 + 0.5 * rng.random(4), max_N=6, lam0=0.25, scheduled=scheduled)
    c0 = float(ref.sum_records(base["span"], base["seg"], base["pair"])[0]) / (3 * base["pair"]["P"])
    trace = []
    for factor in (1.0, 0.5, 0.25, 0.375, 0.25, 0.25 * (1 - 2.0 ** -10), 0.125):
        rec = dict(base, span=base["span"].copy())
        ref.scale_cost(rec, factor)
        info = {}
        before, st = st, ref.gn_step_ref(rec["span"], rec["seg"], rec["pair"], st, args, info)
        trace.append((info["decision"], before, st))
    return c0, trace


def test_state_machine_on_a_scripted_cost_sequence():
    c0, trace = _scripted(conv_tol=1e-2, scheduled=False)
    c = lambda factor: f32(c0 * factor)
    #             decision     lambda   accepted  acc rej flag  done
    expected = [("step",      0.125,   c(1.0),    1,  0,  0,    0),      # first call: no last cost, lambda lowered, step taken
                ("step",      0.0625,  c(0.5),    2,  0,  0,    0),      # down: lambda lowered again
                ("step",      0.03125, c(0.25),   3,  0,  0,    0),      # down
                ("reject",    0.25,    c(0.25),   3,  1,  1,    0),      # up: restored, lambda x 8, flagged
                ("step",      0.25,    c(0.25),   4,  1,  0,    0),      # after a rejection: lambda NOT lowered, step taken
                ("converged", 0.25,    c(0.25),   4,  1,  0,    1),      # down by 2^-10 < 1e-2: done, nothing moves
                ("skip",      0.25,    c(0.25),   4,  1,  0,    1)]      # a done pair is not looked at again
    for k, ((decision, before, after), want) in enumerate(zip(trace, expected)):
        ls = after["lm_state"]
        got = (decision, float(ls[0]), ls[1], int(ls[2]), int(ls[3]), int(ls[4]), after["done"])
        assert got == want, f"call {k}: {got} != {want}"
        moved = not (np.array_equal(before["pose"], after["pose"]) and np.array_equal(before["kld"], after["kld"]))
        assert moved == (decision in ("step", "reject")), f"call {k}"
        if decision == "step":
            assert np.array_equal(after["backup"][:16], before["pose"].ravel()) and np.array_equal(after["backup"][16:20], before["kld"])
            assert np.array_equal(after["backup"][20:], before["backup"][20:])         # beyond N: never written
        if decision == "reject":                                                      # bit for bit what the last step left behind
            assert np.array_equal(after["pose"].ravel(), before["backup"][:16]) and np.array_equal(after["kld"], before["backup"][16:20])
            assert np.array_equal(after["pose"], trace[k - 1][1]["pose"])
    # the last cost SEEN follows every evaluated call, the accepted one does not
    assert [t[2]["lm_state"][5] for t in trace[:6]] == [c(f) for f in (1.0, 0.5, 0.25, 0.375, 0.25, 0.25 * (1 - 2.0 ** -10))]
    assert trace[6][2]["lm_state"][5] == trace[5][2]["lm_state"][5]


def test_state_machine_in_a_schedule_counts_rejections_and_records_how_a_phase_ended():
    _, trace = _scripted(conv_tol=1e-2, scheduled=True)
    want = [(0, 1, 0.0), (0, 2, 0.0), (0, 3, 0.0), (0, 4, 0.0), (0, 5, 0.0), (3, 0, -5.0), (3, 1, -5.0)]
    got = [(t[2]["phase"], t[2]["iters"], float(t[2]["lm_state"][7])) for t in trace]
    assert got == want                                   # the rejected call counts; the converged one leaves with -iterations
    assert trace[5][2]["lm_state"][1] == -1.0 and trace[6][0] == "step"        # the next phase starts afresh: no last cost, a step
    _, trace = _scripted(conv_tol=1e-2, scheduled=True, max_iters=4)
    got = [(t[0], t[2]["phase"], t[2]["iters"], float(t[2]["lm_state"][7]), int(t[2]["lm_state"][4])) for t in trace[:5]]
    assert got == [("step", 0, 1, 0.0, 0), ("step", 0, 2, 0.0, 0), ("step", 0, 3, 0.0, 0), ("reject", 3, 0, 4.0, 0),    # the cap, on a rejection
                   ("step", 3, 1, 4.0, 0)]
    assert float(trace[3][2]["lm_state"][0]) == 0.25     # lambda x 8 stays; the flag does not


def test_frozen_and_clamped_segments_and_the_dropped_pose_block():
    rng = np.random.default_rng(5)
    rec = ref.make_records(rng, 6, [2, 1, 0, 3, 1, 2], n_spans=4, residual_scale=0.25)
    ref.set_segment(rec, 0, h=np.zeros(6), D=4.0, bd=-24.0)          # its own Newton step at lambda = 1: 24 / 8 = +3
    ref.set_segment(rec, 1, D=0.0)                                    # frozen
    ref.set_segment(rec, 4, D=2.5e-13)                                # D (1 + lambda) = 5e-13: frozen
    _, H, bp, _, h, D, bd = ref.sum_records(rec["span"], rec["seg"], rec["pair"])
    dxi, dd, active, info = ref.dense_step(H, bp, h, D, bd, lam=1.0)
    assert active.tolist() == [True, False, False, True, False, True] and info["pose_ok"]
    assert dd[0] == 0.5 and abs(info["unclamped"][0] - 3.0) < 1e-12 and not dd[[1, 2, 4]].any()
    kept = [0, 3, 5]                                                  # the frozen ones are no part of the system at all
    dxi2, dd2, _, _ = ref.dense_step(H, bp, h[kept], D[kept], bd[kept], lam=1.0)
    assert np.array_equal(dxi, dxi2) and np.array_equal(dd[kept], dd2)
    ref.set_segment(rec, 3, h=[40.0, 0, 0, 0, 0, 0], D=1.0, bd=0.25)  # Schur term 1600 / 2 against H_00 of a few hundred
    _, H, bp, _, h, D, bd = ref.sum_records(rec["span"], rec["seg"], rec["pair"])
    dxi, dd, active, info = ref.dense_step(H, bp, h, D, bd, lam=1.0)
    assert not info["pose_ok"] and not dxi.any() and dd[3] == -0.125 and dd[0] == 0.5
    dxi, dd, active, info = ref.dense_step(H, bp, h, D, bd, lam=1.0, pose_only=True)
    assert info["pose_ok"] and not active.any() and not dd.any()
    np.testing.assert_allclose(dxi, np.linalg.solve(H + np.diag(np.diag(H)), -bp), rtol=1e-9)      # LM scales the DIAGONAL
