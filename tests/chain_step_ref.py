"""The yardstick of ONE ``sp_chain_step_multi`` call (include/sp_hip.h; csrc/sp_chain.hip), stage by stage -- numpy, no GPU.

Nothing here is a new reference of an optimiser or a render: the call strings pinned pieces together, and so does this file.  It takes
``compose_edge`` / ``renormalise_rotation`` / ``make_node`` / ``random_pose`` from ``window_gn_step_ref`` and ``make_table`` / ``splat`` /
the taint rule from ``segment_depth_ref``, and adds only what the call does BETWEEN them, restated from the header:

  pack, blur_decimate   the frame's pyramid: level 0 is the planar image permuted, level l >= 1 is [1 2 1; 2 4 2; 1 2 1] / 16 with
                        reflect-1 padding and [::2, ::2] of level l - 1 (a dimension of one pixel reflects onto itself), in float64, with the
                        largest magnitude of every output's 3 x 3 window (the scale of its derived bound);
  set_node              the node overwrite (pose, aff when given; tangent and moments zero);
  fresh_state, rephase  the LM state of a new optimisation / of a new phase;
  slot_moves            the supp_images moves: per element slot 1 -> slot 0 FIRST, then this frame -> slot 1;
  inv_rigid_times       rel = inv(A) B for a rigid A (R^T, -R^T t), float64, and ``rel_pose_bound``, the float32 kernel's derived bound;
  criterion             the four floats of the keyframe criterion from a float32 depth array and two poses;
  run_stepped           the phase loop of a stage as single steps: what part B of tests/test_gpu_chain_step.py runs on a twin window.

Below the line "inputs of the tests" are the seeded render scenes that ``test_chain_step_ref_host.py`` (are they decisive?) and
``test_gpu_chain_step.py`` share."""
import numpy as np

import segment_depth_ref as sd
import window_gn_step_ref as wg
from gn_step_ref import se3_exp

f32 = np.float32
STATE = 16


# ---- the pyramid ----------------------------------------------------------------------------------------------------------------------------
def level_sizes(H, W, n_levels):
    out = [(int(H), int(W))]
    for _ in range(1, n_levels):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def pack(planar):
    """(3,H,W) planar -> (H,W,3) packed: a permutation, no arithmetic."""
    return np.ascontiguousarray(np.transpose(np.asarray(planar), (1, 2, 0)))


def _reflect1_or_self(i, n):
    i = np.asarray(i, np.int64)
    if n == 1:
        return np.zeros_like(i)
    return np.where(i < 0, -i, np.where(i >= n, 2 * n - 2 - i, i))


def blur_decimate(x):
    """One pyramid step of a (C,H,W) float32 image in float64.  Returns (out (C,Ho,Wo), mag (C,Ho,Wo) = the largest |input| under each
    output's window).  The weights are powers of two times 1, 2, 4: every product is exact in float32 and every partial sum is at most
    ``mag`` in magnitude, which is what the bound of the float32 kernel rests on."""
    x = np.asarray(x, f32).astype(np.float64)
    C, H, W = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    w = (1.0, 2.0, 1.0)
    out, mag = np.zeros((C, Ho, Wo)), np.zeros((C, Ho, Wo))
    for dy in range(3):
        rows = _reflect1_or_self(2 * np.arange(Ho) + dy - 1, H)
        for dx in range(3):
            cols = _reflect1_or_self(2 * np.arange(Wo) + dx - 1, W)
            v = x[:, rows][:, :, cols]
            out += w[dy] * w[dx] / 16.0 * v
            mag = np.maximum(mag, np.abs(v))
    return out, mag


BLUR_ULPS = 4         # nine fused multiply-adds from a zero start: the first is an exact product, the other eight round once, half an ulp
#                       each at a partial sum that never exceeds the window's largest magnitude: 8 / 2 = 4 ulp there


# ---- nodes and states -----------------------------------------------------------------------------------------------------------------------
def set_node(nodes, node, pose16, aff=None):
    """The node overwrite in place: T (and aff when a pair is given) from the buffers, tangent and Adam moments zero; lr, kind, flags stay."""
    nd = nodes[node]
    nd["T"] = np.asarray(pose16, f32).ravel()
    if aff is not None:
        nd["aff"] = np.asarray(aff, f32)
    for k in ("a", "m", "v", "aff_m", "aff_v"):
        nd[k] = 0
    return nodes


def fresh_state(lam0):
    st = np.zeros(STATE, f32)
    st[0], st[1] = lam0, -1.0
    return st


def rephase(state):
    """A new phase of the schedule: the accept and convergence tests start afresh, lambda and the iteration count carry over."""
    st = np.array(state, f32)
    st[1], st[4], st[6] = -1.0, 0.0, 0.0
    return st


def slot_moves(slot0, slot1, frame, bits, frame_first=False):
    """(new slot 0, new slot 1).  bit 0: slot 1 -> slot 0; bit 1: this frame -> slot 1.  ``frame_first`` is the WRONG order (the host test
    shows that the two differ exactly when both bits are set)."""
    a, b, t = np.array(slot0), np.array(slot1), np.asarray(frame)
    if frame_first:
        if bits & 2:
            b = np.array(t)
        if bits & 1:
            a = np.array(b)
    else:
        if bits & 1:
            a = np.array(b)
        if bits & 2:
            b = np.array(t)
    return a, b


# ---- inv(A) B -------------------------------------------------------------------------------------------------------------------------------
def inv_rigid_times(A, B):
    """inv(A) B for a RIGID A in float64: inv(A) = [R^T, -R^T t; 0 0 0 1] (lie/lie_algebra.py invertSE3), never a general inverse -- for a
    float32 rotation that is orthonormal only to round-off the two differ by that round-off, and the header states this form."""
    A, B = np.asarray(A, np.float64).reshape(4, 4), np.asarray(B, np.float64).reshape(4, 4)
    inv = np.eye(4)
    inv[:3, :3] = A[:3, :3].T
    inv[:3, 3] = -(A[:3, :3].T @ A[:3, 3])
    return inv @ B


def rel_pose_bound(A, B):
    """Absolute bound (4,4) of the float32 kernel against ``inv_rigid_times``.  Row r < 3 of inv(A): three copies and
    inv[3] = -(three products, two adds): at most 5 roundings of half an ulp at M = sum |R_kr t_k|.  An entry is a four-term dot: 4 products
    and 3 adds, at most 7 roundings of half an ulp at S = sum |inv_k| |B_kc| (M standing for |inv[3]|), plus what inv[3]'s own error
    becomes through |B[3][c]|.  Contraction into fused multiply-adds only removes roundings.  The last row is exact: 0 * x + ... + 1 * B[3][c]."""
    A, B = np.abs(np.asarray(A, np.float64).reshape(4, 4)), np.abs(np.asarray(B, np.float64).reshape(4, 4))
    out = np.zeros((4, 4))
    for r in range(3):
        M = float(A[:3, r] @ A[:3, 3])
        e3 = 2.5 * np.spacing(f32(M))
        for c in range(4):
            S = float(A[:3, r] @ B[:3, c] + M * B[3, c])
            out[r, c] = 3.5 * np.spacing(f32(S)) + e3 * B[3, c]
    return out


# ---- the criterion --------------------------------------------------------------------------------------------------------------------------
CRIT_DIFF_ULPS = 6    # [2]: three float32 differences (relative u = 2^-24 each), squared (2 u) and rounded (+ u), two adds (+ 2 u): 5 u under
#                       the root, which halves it, + u for the root, + u for scale + 1e-6f, + u for the division: 5.5 u <= 5.5 ulp
CRIT_ANGLE_ULPS = 1   # [3]: float64 throughout (products of float32 are exact in float64), rounded once: the nearest float32 or its neighbour


def criterion(depth, thresh, pose_src, pose_trg):
    """(ratio float32, scale float32, diff float64, angle float64, count).  ratio = float32(count) / float32(n) with count = #(depth >
    thresh); scale = the lower median (rank (count - 1) // 2) of those values, NaN without any; diff = |t_src - t_trg| / (scale + 1e-6f);
    angle = the rotation angle of R_src^T R_trg in degrees, atan2(|axis part| / 2, (trace - 1) / 2)."""
    d = np.asarray(depth, f32).ravel()
    with np.errstate(invalid="ignore"):
        vals = np.sort(d[d > f32(thresh)])
    cnt = len(vals)
    ratio = f32(cnt) / f32(d.size)
    scale = vals[(cnt - 1) // 2] if cnt else f32(np.nan)
    S, Tg = np.asarray(pose_src, np.float64).reshape(4, 4), np.asarray(pose_trg, np.float64).reshape(4, 4)
    dt = S[:3, 3] - Tg[:3, 3]
    with np.errstate(all="ignore"):
        diff = np.sqrt(dt @ dt) / (np.float64(scale) + np.float64(f32(1e-6)))
    D = S[:3, :3].T @ Tg[:3, :3]
    ax = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
    angle = np.degrees(np.arctan2(0.5 * np.sqrt(ax @ ax), 0.5 * (np.trace(D) - 1.0)))
    return ratio, f32(scale), float(diff), float(angle), cnt


# ---- the phases of a stage, stepped ---------------------------------------------------------------------------------------------------------
def run_stepped(ops, phases, lam0):
    """The phase loop of a stage from the two pinned calls.  ``ops``: read_state() -> 16 floats, write_state(16 floats), cost(level,
    irls_eps), step(level, conv_tol).  phases: (level, max_iters, irls_eps, conv_tol).  Fresh state; per phase with max_iters > 0 the
    re-phase edit, then cost + step until the state is frozen (state[6]) or max_iters calls were made.  A skipped phase edits nothing.
    Returns the cost + step rounds made in each phase that ran."""
    ops.write_state(fresh_state(lam0))
    rounds = []
    for level, max_iters, eps, tol in phases:
        if max_iters <= 0:
            continue
        ops.write_state(rephase(ops.read_state()))
        rounds.append(0)
        for _ in range(int(max_iters)):
            ops.cost(level, eps)
            ops.step(level, tol)
            rounds[-1] += 1
            if ops.read_state()[6] != 0:
                break
    return rounds


# =============================================================================================================================================
# inputs of the tests (seeded; the host test shows that they are decisive, the GPU test runs the call on them)
# =============================================================================================================================================
# kind: generic = a small motion and a step back (the image shrinks towards the principal point: points pile up); flip = a rotation of 180
# degrees about the optical axis and a step back; behind = everything behind the judged camera (nothing lands); same = the judged pose IS the
# keyframe's (every point re-projects onto its own pixel's corner, u = col exactly: the float64 statement can name no pixel, so this one
# scene is not judged against the render yardstick -- only bitwise against the stand-alone render -- and stands for the criterion's zeros).
# parity: of the number of pixels the yardstick's render touches.
SCENES = {
    "odd18x22": dict(H=18, W=22, N=4, extent=(0.4, 0.8), kind="generic", seed=29, parity=1),
    "even18x22": dict(H=18, W=22, N=3, extent=(0.4, 0.8), kind="generic", seed=12, parity=0),
    "flip18x22": dict(H=18, W=22, N=5, extent=(0.4, 0.8), kind="flip", seed=9, parity=0),
    "behind18x22": dict(H=18, W=22, N=2, extent=(0.4, 0.8), kind="behind", seed=0, parity=0),
    "same18x22": dict(H=18, W=22, N=3, extent=(0.4, 0.8), kind="same", seed=0, parity=None),
    "even16x24": dict(H=16, W=24, N=4, extent=(0.4, 0.8), kind="generic", seed=15, parity=0),
    "granule66x64": dict(H=66, W=64, N=3, extent=(0.15, 0.25), kind="generic", seed=0, parity=None),
    "zero130x128": dict(H=130, W=128, N=3, extent=(0.08, 0.12), kind="generic", seed=0, parity=None),
}
JUDGED = [k for k, v in SCENES.items() if v["kind"] != "same"]
_scenes = {}


def scene(name):
    """One keyframe to render and the pose to judge: masks (N,H,W) bool, L (N,H,W) float32 log-depths, keypoints (N,2) float32 normalised
    (row, col), kld (N,) float32, K (3,3) float32, kf_pose / pose (4,4) float32 (camera to world: the keyframe's and the judged frame's),
    table = ``segment_depth_ref.make_table``.  Depths lie in [1, 2.3]."""
    if name in _scenes:
        return _scenes[name]
    spec = SCENES[name]
    H, W, N = spec["H"], spec["W"], spec["N"]
    rng = np.random.default_rng([spec["seed"], H, W, N])
    masks = np.zeros((N, H, W), bool)
    keypoints = np.zeros((N, 2), f32)
    for n in range(N):
        h, w = (max(2, int(round(rng.uniform(*spec["extent"]) * s))) for s in (H, W))
        r0, c0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        masks[n, r0:r0 + h, c0:c0 + w] = rng.uniform(size=(h, w)) < 0.9
        masks[n, r0, c0] = True
        keypoints[n] = (2.0 * r0 / (H - 1) - 1.0, 2.0 * c0 / (W - 1) - 1.0)
    L = rng.uniform(0.0, np.log(2.0), (N, H, W)).astype(f32)
    table = sd.make_table(masks, L, keypoints)
    kld = (table.kp_L + rng.uniform(-0.1, 0.1, N)).astype(f32)
    K = np.array([[0.9 * W, 0, 0.5 * W + 0.23], [0, 0.9 * W, 0.5 * H - 0.31], [0, 0, 1]], f32)
    kf_pose = wg.random_pose(rng)
    kf_pose[3] = (0, 0, 0, 1)
    kind = spec["kind"]
    if kind == "same":
        pose = kf_pose.copy()
    else:
        if kind == "flip":
            rel = np.diag([-1.0, -1.0, 1.0, 1.0])
            rel[:3, 3] = (0.04, 0.02, 0.9)
        else:
            rel = se3_exp(np.concatenate([rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.04, 0.04, 3)]))
            rel[2, 3] += -10.0 if kind == "behind" else 0.8
        pose = (kf_pose.astype(np.float64) @ np.linalg.inv(rel)).astype(f32)      # rel = inv(pose) kf_pose
        pose[3] = (0, 0, 0, 1)
    _scenes[name] = dict(spec, name=name, masks=masks, L=L, keypoints=keypoints, kld=kld, K=K, kf_pose=kf_pose, pose=pose, table=table)
    return _scenes[name]


def judged_pose(sc, tracked):
    """The pose the criterion judges: the scene's, renormalised when it went through the tracker's read-out."""
    return wg.renormalise_rotation(sc["pose"]).reshape(4, 4) if tracked else sc["pose"]


def render(sc, rel):
    """The render yardstick of a scene under ``rel`` (the device's own rel_pose in the GPU test)."""
    return sd.splat(sc["table"], sc["K"], sc["kld"], np.asarray(rel, np.float64).reshape(4, 4))
