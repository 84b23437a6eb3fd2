"""The yardstick of one ``sp_chain_step_multi`` call (tests/chain_step_ref.py) kept honest without a GPU: its new pieces against
independent statements (torch's float64 convolution, numpy's inverse, the criteria oracle on golden g11), its derived float32 bounds against
the kernels' arithmetic restated in float32, and -- for every render scene ``test_gpu_chain_step.py`` uses -- the conditions under which that
test may demand what it demands.  Every figure is printed before it is asserted (run with -s to see them)."""
import numpy as np
import pytest
import torch

import chain_step_ref as cr
import segment_depth_ref as sd
import window_gn_step_ref as wg
from conftest import load_golden

f32 = np.float32


# ---- the pyramid ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(18, 22), (9, 11), (5, 6), (16, 24), (8, 12), (2, 2), (3, 2), (130, 128)])
def test_pyramid_step_is_torch_s_reflect_padded_convolution(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    x = rng.uniform(-1.0, 1.0, (3, H, W)).astype(f32)
    got, mag = cr.blur_decimate(x)
    k = torch.tensor([[1.0, 2.0, 1.0], [2.0, 4.0, 2.0], [1.0, 2.0, 1.0]], dtype=torch.float64) / 16.0
    xp = torch.nn.functional.pad(torch.from_numpy(x.astype(np.float64))[None], (1, 1, 1, 1), mode="reflect")
    want = torch.nn.functional.conv2d(xp, k[None, None].repeat(3, 1, 1, 1), groups=3)[0, :, ::2, ::2].numpy()
    assert got.shape == want.shape == (3, (H + 1) // 2, (W + 1) // 2)
    assert np.abs(got - want).max() <= 1e-15
    assert (np.abs(got) <= mag + 1e-15).all() and (mag <= np.abs(x).max()).all()
    # the kernel's arithmetic restated in float32 (nine fused multiply-adds from zero, emulated by a float64 product-sum rounded once per
    # step) stays inside the derived bound
    acc = np.zeros(got.shape, f32)
    for dy in range(3):
        rows = cr._reflect1_or_self(2 * np.arange(got.shape[1]) + dy - 1, H)
        for dx in range(3):
            cols = cr._reflect1_or_self(2 * np.arange(got.shape[2]) + dx - 1, W)
            wgt = (1.0, 2.0, 1.0)[dy] * (1.0, 2.0, 1.0)[dx] / 16.0
            acc = (wgt * x[:, rows][:, :, cols].astype(np.float64) + acc.astype(np.float64)).astype(f32)
    d = (np.abs(acc - got) / np.spacing(np.maximum(mag, 1e-30).astype(f32))).max()
    print(f"\n{H}x{W}: float32 restatement off by {d:.2f} ulp at the window's largest magnitude (bound {cr.BLUR_ULPS})")
    assert d <= cr.BLUR_ULPS


def test_a_dimension_of_one_pixel_reflects_onto_itself_and_packing_permutes():
    x = np.arange(3, dtype=f32).reshape(3, 1, 1) + 0.5
    out, mag = cr.blur_decimate(x)
    assert np.array_equal(out, x) and np.array_equal(mag, x)
    row, _ = cr.blur_decimate(np.arange(12, dtype=f32).reshape(3, 1, 4))          # one row: the vertical taps all read it
    assert np.allclose(row[0, 0], [(2 * 0 + 2 * 1) / 4.0, (1 + 2 * 2 + 3) / 4.0])
    p = np.arange(24, dtype=f32).reshape(3, 2, 4)
    q = cr.pack(p)
    assert q.shape == (2, 4, 3) and all(q[r, c, ch] == p[ch, r, c] for r in range(2) for c in range(4) for ch in range(3))
    assert cr.level_sizes(18, 22, 3) == [(18, 22), (9, 11), (5, 6)] and cr.level_sizes(2, 2, 2) == [(2, 2), (1, 1)]


# ---- inv(A) B -------------------------------------------------------------------------------------------------------------------------------
def _kernel_rel_pose(A, B):
    """k_chain_rel_pose_multi operation by operation in float32 (no contraction: the most roundings the compiler may leave)."""
    A, B = np.asarray(A, f32).ravel(), np.asarray(B, f32).ravel()
    out = np.zeros(16, f32)
    for t in range(16):
        r, c = t >> 2, t & 3
        if r < 3:
            inv = [A[r], A[4 + r], A[8 + r]]
            inv.append(-((inv[0] * A[3] + inv[1] * A[7]) + inv[2] * A[11]))
        else:
            inv = [f32(0), f32(0), f32(0), f32(1)]
        out[t] = ((inv[0] * B[c] + inv[1] * B[4 + c]) + inv[2] * B[8 + c]) + inv[3] * B[12 + c]
    return out.reshape(4, 4)


def test_rel_pose_is_numpy_s_inverse_on_rigid_poses_and_its_bound_covers_float32():
    from gn_step_ref import se3_exp
    rng = np.random.default_rng(77)
    worst = 0.0
    for k in range(200):
        A64 = se3_exp(np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-2, 2, 3)]))
        B64 = se3_exp(np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-2, 2, 3)]))
        A64[3] = B64[3] = (0, 0, 0, 1)
        assert np.abs(cr.inv_rigid_times(A64, B64) - np.linalg.inv(A64) @ B64).max() <= 1e-13
        A, B = A64.astype(f32), B64.astype(f32)
        want, bound = cr.inv_rigid_times(A, B), cr.rel_pose_bound(A, B)
        got = _kernel_rel_pose(A, B)
        assert np.array_equal(got[3], [0, 0, 0, 1]) and not bound[3].any() and (bound[:3] > 0).all()
        worst = max(worst, (np.abs(got - want)[:3] / bound[:3]).max())
        # rows and columns of the rotation exchanged is far outside the bound
        wrong = np.array(A)
        wrong[:3, :3] = A[:3, :3].T
        assert (np.abs(cr.inv_rigid_times(wrong, B) - want) > 1e3 * bound).any()
    print(f"\nfloat32 restatement of inv(A) B: at most {worst:.3f} of the derived bound")
    assert worst <= 1.0


# ---- the criterion --------------------------------------------------------------------------------------------------------------------------
def test_criterion_is_the_oracle_s_on_golden_g11():
    from oracle import kf_oracle
    g = load_golden("g11_kf_criteria")
    for tag in ("odd", "even", "dense", "one"):
        a, b, d = g[f"{tag}_pose_src"], g[f"{tag}_pose_trg"], g[f"{tag}_depth"]
        ratio, scale, diff, angle, cnt = cr.criterion(d, 1e-6, a, b)
        ta, tb, td = (torch.from_numpy(np.ascontiguousarray(x)) for x in (a, b, d))
        want_diff, want_scale = kf_oracle.translation_difference(ta, tb, td)
        assert cnt == int(g[f"{tag}_n_valid"]) and scale == float(g[f"{tag}_scale"]) == float(want_scale)
        assert ratio == f32(cnt) / f32(d.size) and abs(float(ratio) - float(kf_oracle.validity_ratio(td))) <= 1e-7
        np.testing.assert_allclose(diff, float(g[f"{tag}_diff"]), rtol=2e-6)
        np.testing.assert_allclose(diff, float(want_diff), rtol=2e-6)
        np.testing.assert_allclose(angle, float(g[f"{tag}_angle_deg"]), rtol=2e-5, atol=1e-4)
        np.testing.assert_allclose(angle, kf_oracle.rotation_difference(ta, tb), rtol=2e-5, atol=1e-4)


def test_criterion_edges_written_out_by_hand():
    I = np.eye(4, dtype=f32)
    Rz = np.diag([-1.0, -1.0, 1.0, 1.0]).astype(f32)
    moved = I.copy()
    moved[:3, 3] = (3, 0, 4)
    d = np.array([np.nan, -1.0, 0.0, 1e-6, 2.0, 4.0, 8.0, np.inf], f32)
    ratio, scale, diff, angle, cnt = cr.criterion(d, 1e-6, I, I)
    assert cnt == 4 and ratio == f32(0.5) and scale == 4.0 and diff == 0.0 and angle == 0.0      # NaN, negative, 0 and thresh itself are out
    ratio, scale, diff, angle, cnt = cr.criterion(d[:7], 1e-6, moved, Rz)
    assert cnt == 3 and scale == 4.0 and abs(diff - 5.0 / (4.0 + float(f32(1e-6)))) < 1e-15 and angle == 180.0
    ratio, scale, diff, angle, cnt = cr.criterion(np.zeros(5, f32), 1e-6, moved, I)
    assert cnt == 0 and ratio == 0 and np.isnan(scale) and np.isnan(diff) and angle == 0.0
    ratio, scale, diff, angle, cnt = cr.criterion(np.array([0.0, 1e-42, 3.0], f32), 0.0, I, I)      # thresh = 0: a denormal is valid
    assert cnt == 2 and scale == f32(1e-42)
    assert cr.criterion(np.array([1.0, 2.0, 3.0, 4.0], f32), 0.5, I, I)[1] == 2.0                   # even count: the LOWER middle


# ---- the render scenes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tracked", [False, True], ids=["judged as given", "judged after the read-out"])
@pytest.mark.parametrize("name", cr.JUDGED)
def test_render_scenes_are_decisive(name, tracked):
    sc = cr.scene(name)
    t = sc["table"]
    A = cr.judged_pose(sc, tracked)
    rel = cr.inv_rigid_times(A, sc["kf_pose"])
    r = cr.render(sc, rel)
    qz32, u32, v32 = sd.positions(t, sc["K"], sc["kld"], rel, np.float32)
    near = (r.qz > sd.EPS) & (r.u > -2) & (r.u < sc["W"] + 1) & (r.v > -2) & (r.v < sc["H"] + 1)
    du, dv = np.abs(u32 - r.u)[near].max(initial=0.0), np.abs(v32 - r.v)[near].max(initial=0.0)
    touched = int((r.count > 0).sum())
    collisions = int(((r.count >= 2) & ~r.taint).sum())
    print(f"\n{name}: {t.P} points of {t.N} segments, {touched} pixels touched, {collisions} untainted pixels hit more than once, tainted "
          f"{r.taint.mean():.4f}, float32 gap du {du:.2e} dv {dv:.2e} px")
    assert sd.DELTA == 1e-3 and du <= sd.DELTA / 16 and dv <= sd.DELTA / 16
    assert r.taint.mean() <= 0.02
    assert not np.any(np.abs(r.qz - sd.EPS) < 1e-5)
    if sc["H"] * sc["W"] < 1000:
        assert not r.taint.any()                      # the small frames: no ambiguous point at all, so the count of valid pixels is decided
    if sc["kind"] == "behind":
        assert touched == 0 and not (r.qz > 0).any()
    else:
        assert collisions >= 1 and touched >= 20
        assert (r.image[r.count > 0] > 0.5).all()     # far above valid_thresh
    if sc["parity"] is not None:
        assert touched % 2 == sc["parity"]
    if sc["kind"] == "flip":
        assert abs(cr.criterion(r.image, 1e-6, A, sc["kf_pose"])[3] - 180.0) < 1e-3
    assert t.P <= 700 and t.P % 256


def test_scene_of_identical_poses_cannot_be_judged_by_the_render_yardstick():
    sc = cr.scene("same18x22")
    assert np.array_equal(sc["pose"], sc["kf_pose"])
    r = cr.render(sc, cr.inv_rigid_times(sc["pose"], sc["kf_pose"]))
    assert r.ambiguous[r.pix >= 0].mean() > 0.9                                     # u = col: every point sits on a pixel corner
    assert cr.criterion(r.image, 1e-6, sc["pose"], sc["kf_pose"])[2:4] == (0.0, 0.0)


def test_scenes_of_one_frame_size_differ_in_P_and_N():
    same = [cr.scene(n) for n in cr.SCENES if n.endswith("18x22")]
    assert len({s["table"].P for s in same}) == len(same) and len({s["N"] for s in same}) >= 3
    assert 66 * 64 > 4096 and 130 * 128 > 64 * 256


# ---- the slot moves -------------------------------------------------------------------------------------------------------------------------
def test_slot_move_reference_distinguishes_the_two_orders():
    a, b, t = np.full(5, 1.0, f32), np.full(5, 2.0, f32), np.full(5, 3.0, f32)
    want = {0: (1, 2), 1: (2, 2), 2: (1, 3), 3: (2, 3)}
    for bits, (s0, s1) in want.items():
        got = cr.slot_moves(a, b, t, bits)
        assert (got[0] == s0).all() and (got[1] == s1).all()
        other = cr.slot_moves(a, b, t, bits, frame_first=True)
        same = np.array_equal(other[0], got[0]) and np.array_equal(other[1], got[1])
        assert same == (bits != 3)
    assert (cr.slot_moves(a, b, t, 3, frame_first=True)[0] == 3).all()             # the wrong order loses the old slot 1
    assert (a == 1).all() and (b == 2).all()                                        # the inputs are not edited


# ---- nodes and states -----------------------------------------------------------------------------------------------------------------------
def test_node_overwrite_and_states():
    rng = np.random.default_rng(3)
    nodes = np.array([wg.make_node(T=wg.random_pose(rng), aff=(0.25, -0.5), kind=k, flags=k, a=(1, 2, 3, 4, 5, 6)) for k in (0, 1)], wg.NODE)
    before = nodes.copy()
    pose = wg.random_pose(rng)
    cr.set_node(nodes, 1, pose.ravel(), None)
    assert nodes[0].tobytes() == before[0].tobytes()
    assert np.array_equal(nodes[1]["T"], pose.ravel()) and np.array_equal(nodes[1]["aff"], before[1]["aff"])
    assert not any(nodes[1][k].any() for k in ("a", "m", "v", "aff_m", "aff_v"))
    assert all(nodes[1][k] == before[1][k] for k in ("lr_pose", "lr_aff", "kind", "flags"))
    cr.set_node(nodes, 0, pose.ravel(), (0.5, 1.5))
    assert np.array_equal(nodes[0]["aff"], [0.5, 1.5])
    st = cr.fresh_state(2.5)
    assert st.dtype == f32 and st.tolist() == [2.5, -1.0] + [0.0] * 14
    busy = np.arange(16, dtype=f32) + 1
    re = cr.rephase(busy)
    assert re[1] == -1 and re[4] == 0 and re[6] == 0 and np.array_equal(np.delete(re, [1, 4, 6]), np.delete(busy, [1, 4, 6])) and busy[1] == 2


# ---- the stepped driver against a stub ------------------------------------------------------------------------------------------------------
class _Stub:
    """A window that halves lambda on every step, counts its steps in state[5], stores the loss in state[1], marks a reject streak in
    state[4] and freezes (state[6]) after ``freeze_after[phase]`` steps of a phase; once frozen a step does nothing."""

    def __init__(self, freeze_after):
        self.state = np.full(16, 99.0, f32)
        self.freeze_after, self.log, self.phase, self.in_phase, self.pending = freeze_after, [], -1, 0, None

    def read_state(self):
        return self.state.copy()

    def write_state(self, st):
        st = np.asarray(st, f32)
        assert st.shape == (16,)
        self.log.append(("rephase" if self.log else "fresh", st.copy()))
        if self.log[-1][0] == "rephase":
            self.phase += 1
            self.in_phase = 0
        self.state = st.copy()

    def cost(self, level, eps):
        assert self.pending is None
        self.pending = (level, eps)

    def step(self, level, tol):
        assert self.pending is not None and self.pending[0] == level
        self.log.append(("round", level, self.pending[1], tol))
        self.pending = None
        if self.state[6] != 0:
            return
        self.in_phase += 1
        self.state[0] *= f32(0.5)
        self.state[1], self.state[4] = 7.0, 1.0
        self.state[5] += 1
        if self.in_phase >= self.freeze_after[self.phase]:
            self.state[6] = 1.0


def test_stepped_driver_keeps_the_phase_and_state_books():
    phases = [(1, 4, 1e-3, 2e-3), (2, 0, 5e-3, 1e-3), (0, 6, 1e-5, 1e-4), (0, 2, 1e-5, 0.0)]
    stub = _Stub(freeze_after=[2, 99, 99])
    rounds = cr.run_stepped(stub, phases, lam0=0.25)
    kinds = [e[0] for e in stub.log]
    # fresh; phase 0 frozen after 2 of 4; the max_iters = 0 phase neither runs nor edits; phase 2 its full 6; phase 3 its 2
    assert kinds == ["fresh", "rephase", "round", "round", "rephase"] + ["round"] * 6 + ["rephase", "round", "round"] and rounds == [2, 6, 2]
    assert stub.log[0][1].tolist() == [0.25, -1.0] + [0.0] * 14
    assert [e[1:] for e in stub.log if e[0] == "round"] == [(1, 1e-3, 2e-3)] * 2 + [(0, 1e-5, 1e-4)] * 6 + [(0, 1e-5, 0.0)] * 2
    second = stub.log[4][1]                          # the state the second running phase starts from
    assert second[0] == f32(0.25) / 4 and second[5] == 2 and second[1] == -1 and second[4] == 0 and second[6] == 0
    assert stub.state[5] == 10 and stub.state[0] == f32(0.25) / 1024 and stub.state[6] == 0
    # no phase at all: the fresh state and nothing else
    none = _Stub(freeze_after=[])
    assert cr.run_stepped(none, [(0, 0, 1e-3, 1e-3), (1, -1, 1e-3, 1e-3)], lam0=1.5) == []
    assert [e[0] for e in none.log] == ["fresh"] and none.state.tolist() == [1.5, -1.0] + [0.0] * 14
