"""The float64 yardstick of one sp_window_gn_step call (tests/window_gn_step_ref.py) checked against independent statements of the same
things, without a GPU: the chain rule z_e = G [y_trg ; y_src] against finite differences of the relative pose (the oracle's SE(3)
exponential), its dense step against a least-squares solve of the rows the records were made from, its LM state machine against a
sequence written out by hand, its reading of the mode-2 records against the index map of
test_gpu_window_gn.py::test_mode2_normal_equations_with_affine_columns_match_oracle_jacobian."""
import numpy as np
import pytest
import torch

import window_gn_step_ref as ref
from window_gn_step_ref import WinArgs, f32


def _exp(xi):
    from oracle.photometric_oracle import se3_exp
    return se3_exp(torch.from_numpy(np.asarray(xi, np.float64))).numpy()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_chain_rule_by_finite_differences_of_the_relative_pose(seed):
    """inv(T_t Exp(-d_t)) (T_s Exp(-d_s)) = Exp(G [d_t ; d_s]) M to first order, M = inv(T_t) T_s: the sign and the side of Ad."""
    rng = np.random.default_rng(seed)
    Tt, Ts = (ref.random_pose(rng).astype(np.float64) for _ in range(2))
    M = np.linalg.inv(Tt) @ Ts
    nodes = np.array([ref.make_node(T=Tt, lr_aff=0.0), ref.make_node(T=Ts, lr_aff=0.0)], ref.NODE)          # y = [d_t (6) ; d_s (6)]
    G = ref.edge_map((1, 0, 0, 1.0), nodes, M)[:6]
    assert G.shape == (6, 12) and np.array_equal(G[:, :6], np.eye(6))
    rel = lambda d: np.linalg.inv(Tt @ _exp(-d[:6])) @ (Ts @ _exp(-d[6:]))
    h = 1e-4          # central differences: truncation ~ h^2 / 6 = 2e-9, rounding of the oracle's closed form ~ 1e-13 / h
    for k in range(12):
        e = np.zeros(12)
        e[k] = h
        moved = (rel(e) - rel(-e)) / (2 * h)
        claimed = (_exp(G @ e) @ M - _exp(-G @ e) @ M) / (2 * h)
        np.testing.assert_allclose(moved, claimed, rtol=0, atol=1e-7, err_msg=f"direction {k}")
    # the wrong sign / the transpose are far away (what the tolerance above separates)
    e = np.zeros(12)
    e[6:] = h
    moved = (rel(e) - rel(-e)) / (2 * h)
    for wrong in (-G[:, 6:], G[:, 6:].T):
        assert np.abs(moved - (_exp(wrong @ e[6:]) @ M - _exp(-wrong @ e[6:]) @ M) / (2 * h)).max() > 1e-2


def small_window(rng, exact=True):
    """Four nodes (0 fixed, 1 and 2 free pose + affine, 3 pose only), two blocks, five edges with shared nodes, one src_node = -1."""
    nodes = [ref.make_node(T=ref.random_pose(rng), lr_pose=0.0, lr_aff=0.0, aff=(0.02, -0.01)),
             ref.make_node(T=ref.random_pose(rng), aff=(0.03, 0.01)), ref.make_node(T=ref.random_pose(rng), aff=(-0.02, 0.04)),
             ref.make_node(T=ref.random_pose(rng), lr_aff=0.0)]
    edges = [(0, 1, 0, 1.0), (0, 2, 0, 0.5), (1, 2, 1, 1.0), (2, 1, 1, 2.0), (-1, 3, 1, 1.0), (1, 3, 1, 1.0)]
    blocks = [(3, 1.0), (4, 1.0)]
    recs = [ref.make_window_records(rng, blocks[e[2]][0], [2, 1, 3, 2][:blocks[e[2]][0]], 3, exact=exact) for e in edges]
    span, seg, pairs = ref.lay_out(recs)
    win = dict(edges=edges, blocks=blocks, pairs=pairs)
    nodes = np.array(nodes, ref.NODE)
    slots = [ref.compose_edge(e, nodes) for e in edges]
    return win, nodes, recs, span, seg, [s[0] for s in slots], [s[1] for s in slots]


@pytest.mark.parametrize("exact", [True, False])
def test_undamped_step_is_the_least_squares_solution_of_the_rows(exact):
    rng = np.random.default_rng(17)
    win, nodes, recs, span, seg, poses, _ = small_window(rng, exact)
    systems = [ref.edge_system(span, seg, p, e[3]) for p, e in zip(win["pairs"], win["edges"])]
    H, b, ny, free = ref.assemble(win, nodes, poses, systems, 0)
    assert ny == 22 and free.all()
    dy, dd, active, info = ref.dense_step(H, b, ny, free, 0.0)
    assert active.all() and info["ok"] and info["cond"] <= 1e6
    assert np.abs(info["unclamped"]).max() < 0.5, "a clamp is active: choose a smaller residual_scale"
    want_y, want_d = ref.lstsq_step(win, nodes, poses, recs)
    scale = max(np.abs(want_y).max(), np.abs(want_d).max())
    tol = 1e-9 if exact else 1e-5          # (not exact: the records are the rows' sums ROUNDED to float32)
    np.testing.assert_allclose(dy, want_y, rtol=tol, atol=tol * scale)
    np.testing.assert_allclose(dd, want_d, rtol=tol, atol=tol * scale)
    # flags bit 0: the depths are no unknowns, the cameras step alone
    H, b, ny, free = ref.assemble(win, nodes, poses, systems, 1)
    dy, dd, active, info = ref.dense_step(H, b, ny, free, 0.0)
    want_y, want_d = ref.lstsq_step(win, nodes, poses, recs, flags=1)
    assert not active.any() and not dd.any() and not want_d.any()
    np.testing.assert_allclose(dy, want_y, rtol=tol, atol=tol * np.abs(want_y).max())


def test_state_machine_on_a_scripted_loss_sequence():
    """loss: 1 (first call) -> 1/2 (down) -> 3/4 (up) -> 1/2 again at the restored point -> 1/2 (1 - 2^-10) (down by less than the
    tolerance) -> anything: accept, accept, reject, accept, converge, frozen."""
    rng = np.random.default_rng(23)
    win, nodes, recs, span, seg, poses, affs = small_window(rng)
    args = WinArgs(lm_up=8.0, lm_down=0.5, lm_min=1e-7, conv_tol=1e-2, n_unknowns=22, max_losses=4)
    st = ref.new_state(nodes, [0.0625 * rng.integers(-4, 5, N) for N, _ in win["blocks"]], poses, affs, lam0=0.25, losses_len=6)
    base = span.copy()
    trace = []
    for factor in (1.0, 0.5, 0.75, 0.5, 0.5 * (1 - 2.0 ** -10), 0.125):
        span = base.copy()
        for p in win["pairs"]:
            span[p["tile0"]:p["tile0"] + p["n_tiles"], 0] = (base[p["tile0"]:p["tile0"] + p["n_tiles"], 0].astype(np.float64) * factor).astype(f32)
        info = {}
        before, st = st, ref.window_gn_step_ref(span, seg, win, st, args, info)
        trace.append((info, before, st))
    def L(factor):          # straight from the rows (dyadic: sum |r| x factor is exact in the float32 records)
        total = 0.0
        for e, r in zip(win["edges"], recs):
            total += e[3] * ((np.abs(r["rows"][3]).sum() * factor) * (1.0 / (3.0 * r["pair"]["P"])))
        return f32(total)
    #            decision     lambda   accepted loss  acc rej flag its frozen last loss
    expected = [("step",      0.125,   L(1.0),        1,  0,  0,   1,  0,     L(1.0)),
                ("step",      0.0625,  L(0.5),        2,  0,  0,   2,  0,     L(0.5)),
                ("reject",    0.5,     L(0.5),        2,  1,  1,   3,  0,     L(0.75)),        # restored, lambda x 8, flagged
                ("step",      0.5,     L(0.5),        3,  1,  0,   4,  0,     L(0.5)),         # after a rejection: lambda NOT lowered, no test
                ("converged", 0.5,     L(0.5),        3,  1,  0,   5,  1,     L(0.5 * (1 - 2.0 ** -10))),
                ("frozen",    0.5,     L(0.5),        3,  1,  0,   5,  1,     L(0.5 * (1 - 2.0 ** -10)))]
    for k, ((info, before, after), want) in enumerate(zip(trace, expected)):
        s = after["state"]
        got = (info["decision"], float(s[0]), s[1], int(s[2]), int(s[3]), int(s[4]), int(s[5]), int(s[6]), s[7])
        assert got == want, f"call {k}: {got} != {want}"
        assert not s[8:].any()
        flat = lambda v: b"".join(np.asarray(x).tobytes() for x in (v if isinstance(v, list) else [v]))
        same = lambda key: flat(before[key]) == flat(after[key])
        moved = not (same("nodes") and same("klds") and same("pose") and same("aff"))
        assert moved == (info["decision"] in ("step", "reject")), f"call {k}"
        if info["decision"] == "step":             # the backups hold the point left
            assert np.array_equal(after["nodes_backup"], before["nodes"]) and np.array_equal(after["kld_backup"], np.concatenate(before["klds"]))
        else:
            assert same("nodes_backup") and same("kld_backup")
        if info["decision"] == "reject":           # bit for bit the point the last step left
            assert np.array_equal(after["nodes"], trace[k - 1][1]["nodes"]) and same("nodes_backup")
            assert all(np.array_equal(x, y) for x, y in zip(after["klds"], trace[k - 1][1]["klds"]))
            assert np.array_equal(after["pose"], trace[k - 1][1]["pose"]) and np.array_equal(after["aff"], trace[k - 1][1]["aff"])
    # losses[]: one per evaluated call, none beyond max_losses, the iteration count goes on
    assert trace[-1][2]["losses"].tolist() == [L(1.0), L(0.5), L(0.75), L(0.5), -5.0, -5.0]


def test_too_many_unknowns_failed_factorisation_and_predicted_exit():
    rng = np.random.default_rng(29)
    win, nodes, recs, span, seg, poses, affs = small_window(rng)
    klds = [np.zeros(N, f32) for N, _ in win["blocks"]]
    st0 = ref.new_state(nodes, klds, poses, affs, lam0=2.0)
    info = {}
    st = ref.window_gn_step_ref(span, seg, win, st0, WinArgs(n_unknowns=21), info)
    assert info["decision"] == "too_many" and st["state"][9] == 1 and st["state"][6] == 1
    st["state"][[6, 9]] = 0
    assert all(np.array_equal(np.asarray(st[k]), np.asarray(st0[k])) for k in ("nodes", "nodes_backup", "kld_backup", "pose", "aff", "state", "losses"))
    # a negative lambda makes the damped camera diagonal negative: nothing moves, lambda x lm_up, [8] counts, [4] is set, [2] and [3] stay
    st0["state"][0] = -3.0
    args = WinArgs(n_unknowns=22, lm_up=-1e-4, lm_down=1.0, lm_min=-10.0, conv_tol=1e-2, flags=2)
    st = ref.window_gn_step_ref(span, seg, win, st0, args, info)
    assert info["decision"] == "failed" and st["state"].tolist()[:10] == [float(f32(-3.0) * f32(-1e-4)), st["state"][7], 0, 0, 1, 1, 0, st["state"][7], 1, 0]
    assert np.array_equal(st["nodes"], st0["nodes"]) and np.array_equal(st["nodes_backup"], st0["nodes"])
    st2 = ref.window_gn_step_ref(span, seg, win, st, args, info)           # the same point again: no convergence test, lambda not lowered: a step
    assert info["decision"] == "step" and st2["state"][0] == st["state"][0] and st2["state"][2] == 1 and st2["state"][4] == 0
    # predicted exit: the gain is -(b . delta); it freezes a step at lambda <= 1e-2 only
    for lam0, tol, frozen in ((2e-4, 1e3, 1), (2e-4, 1e-9, 0), (0.2, 1e3, 0)):
        st0["state"][0] = lam0
        st = ref.window_gn_step_ref(span, seg, win, st0, WinArgs(n_unknowns=22, conv_tol=tol, flags=2), info)
        assert info["decision"] == "step" and info["gain"] > 0 and st["state"][6] == frozen, (lam0, tol)
        want = -(info["b"][:22] @ info["dy"]) - info["b"][22:][info["active"]] @ info["dd"][info["active"]]
        assert info["gain"] == want


def test_record_layout_agrees_with_the_cost_pass_test():
    """x = [xi (6), kld (N), a_t, b_t] as tests/test_gpu_window_gn.py:44-59 fills H and b from the records, here for N = 1."""
    rng = np.random.default_rng(31)
    s, q = rng.standard_normal(48), rng.standard_normal(12)
    iu = np.triu_indices(6)
    N = 1
    H = np.zeros((8 + N, 8 + N))
    b = np.zeros(8 + N)
    Hpp = np.zeros((6, 6)); Hpp[iu] = s[1:22]
    H[:6, :6] = Hpp + np.triu(Hpp, 1).T
    b[:6] = s[22:28]
    A, B = 6 + N, 7 + N
    H[A, A], H[A, B], H[B, A], H[B, B] = s[29], s[30], s[30], s[31]
    b[A], b[B] = s[32], s[33]
    H[:6, A] = H[A, :6] = s[34:40]
    H[:6, B] = H[B, :6] = s[40:46]
    n = 6
    H[:6, n] += q[0:6]; H[n, :6] += q[0:6]
    H[n, n] += q[6]; b[n] += q[7]
    H[n, A] += q[8]; H[A, n] += q[8]; H[n, B] += q[9]; H[B, n] += q[9]
    sr, Hz, bz, valid = ref.read_span(s)
    c, D, bd = ref.read_seg(q)
    z = [0, 1, 2, 3, 4, 5, A, B]
    assert sr == s[0] and valid == s[28]
    assert np.array_equal(Hz, H[np.ix_(z, z)]) and np.array_equal(bz, b[z])
    assert np.array_equal(c, H[n, z]) and D == H[n, n] and bd == b[n]


def test_renormalisation_restated_in_float32():
    rng = np.random.default_rng(37)
    for _ in range(8):
        T = ref.random_pose(rng, scale=4.0)
        T[:3, :3] += (1e-4 * rng.standard_normal((3, 3))).astype(f32)
        R = ref.renormalise_rotation(T.ravel()).reshape(4, 4)
        assert R.dtype == f32 and np.array_equal(R[:, 3], T[:, 3]) and np.array_equal(R[3], T[3])
        np.testing.assert_allclose(R[:3, :3].astype(np.float64) @ R[:3, :3].T, np.eye(3), atol=ref.RENORM_OPS * 2.0 ** -24)
        np.testing.assert_allclose(R[:3, :3], T[:3, :3], atol=1e-3)
