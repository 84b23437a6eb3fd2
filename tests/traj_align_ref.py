"""Float64 numpy restatement of the reference's trajectory alignment (tool/pose_utils.py ``align`` :71-133, ``transfer_scale`` :16-48,
``apply_scale`` :50-68), written from their semantics, and the shared cases of the alignment tests.

``align_poses`` is what ``sp_traj_align`` computes per trajectory: every field of the ``SpTrajAlign`` record plus the per-pose errors.
The decomposition is numpy's SVD (LAPACK gesdd, as in the reference); sums run in pose order."""
import numpy as np


def align(model, data):
    """model, data: (3, n) float64.  The reference's dictionary, plus ``dots``, ``norms``, ``sigma`` (the singular values) and
    ``reflected`` (whether the det fix applied)."""
    model, data = np.asarray(model, np.float64), np.asarray(data, np.float64)
    mm, dm = model.mean(1, keepdims=True), data.mean(1, keepdims=True)
    mz, dz = model - mm, data - dm
    W = np.zeros((3, 3))
    for i in range(model.shape[1]):
        W += np.outer(mz[:, i], dz[:, i])
    U, sigma, Vh = np.linalg.svd(W.T)
    S = np.eye(3)
    reflected = bool(np.linalg.det(U) * np.linalg.det(Vh) < 0)
    if reflected:
        S[2, 2] = -1.0
    rot = U @ S @ Vh
    rotmodel = rot @ mz
    dots = norms = 0.0
    for i in range(model.shape[1]):
        dots += float(dz[:, i] @ rotmodel[:, i])
        ni = np.linalg.norm(mz[:, i])
        norms += ni * ni
    s = float(dots / norms)
    trans_scaled = dm - s * (rot @ mm)
    trans = dm - rot @ mm
    aligned_scaled = s * (rot @ model) + trans_scaled
    aligned = rot @ model + trans
    return {'rot': rot, 'trans_scaled': trans_scaled, 'trans_scaled_error': np.sqrt(((aligned_scaled - data) ** 2).sum(0)),
            'trans': trans, 'trans_error': np.sqrt(((aligned - data) ** 2).sum(0)), 's': s, 'model_aligned_scaled': aligned_scaled,
            'model_aligned': aligned, 'dots': dots, 'norms': norms, 'sigma': sigma, 'reflected': reflected}


def transfer_scale(gt_poses, est_poses, anchor_rotation=False):
    gt = [np.array(p, dtype=np.float64) for p in gt_poses]
    est = [np.array(p, dtype=np.float64) for p in est_poses]
    assert len(gt) == len(est) > 0
    reanchor = gt[0][:3, :3] @ est[0][:3, :3].T
    a = align(np.stack([p[:3, 3] for p in est], axis=1), np.stack([p[:3, 3] for p in gt], axis=1))
    for i, p in enumerate(est):
        p[:3, 3] = a['model_aligned_scaled'][:, i]
        p[:3, :3] = reanchor @ p[:3, :3]
    if anchor_rotation:
        a['rot_reanchor'] = reanchor
    return est, a


def apply_scale(T, pose_align):
    T = np.array(T, dtype=np.float64)
    T[:3, 3] = pose_align['s'] * (pose_align['rot'] @ T[:3, 3]) + np.asarray(pose_align['trans_scaled']).reshape(3)
    if 'rot_reanchor' in pose_align:
        T[:3, :3] = pose_align['rot_reanchor'] @ T[:3, :3]
    return T


FIELDS = ('rot', 'trans_scaled', 'trans', 's', 'rot_reanchor', 'ate_scaled', 'ate', 'dots', 'norms', 'sigma', 'trans_scaled_error', 'trans_error')


def align_poses(pred, gt, anchor_rotation=False):
    """pred, gt: (n, 4, 4).  Every output of ``sp_traj_align`` for one trajectory, float64: the fields of the record and the per-pose errors."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    a = align(pred[:, :3, 3].T, gt[:, :3, 3].T)
    return dict(rot=a['rot'], trans_scaled=a['trans_scaled'].reshape(3), trans=a['trans'].reshape(3), s=np.float64(a['s']),
                rot_reanchor=gt[0, :3, :3] @ pred[0, :3, :3].T if anchor_rotation else np.eye(3),
                ate_scaled=np.sqrt(np.mean(a['trans_scaled_error'] ** 2)), ate=np.sqrt(np.mean(a['trans_error'] ** 2)),
                dots=np.float64(a['dots']), norms=np.float64(a['norms']), sigma=a['sigma'], trans_scaled_error=a['trans_scaled_error'],
                trans_error=a['trans_error'])


def condition(pred, gt):
    """(sigma_2 - sigma_3) / sigma_1 of the cross-covariance: how well the rotation about the dominant axis pair is determined.  (The
    rotation is unique while sigma_2 > sigma_3 -- with the det fix sigma_3's sign is free --, so this is the gap that matters.)"""
    sigma = align_poses(pred, gt)['sigma']
    return float((sigma[1] - sigma[2]) / sigma[0])


def permutation_spread(pred, gt, anchor_rotation=False, n_perm=8, seed=0):
    """Per field, the largest deviation of the restatement on ``n_perm`` random orders of the poses from the given order (per-pose
    errors compared pose by pose; the first pose stays first: it anchors ``rot_reanchor``)."""
    base = align_poses(pred, gt, anchor_rotation)
    rng = np.random.default_rng(seed)
    spread = {k: 0.0 for k in FIELDS}
    n = len(pred)
    for _ in range(n_perm):
        p = np.concatenate(([0], 1 + rng.permutation(n - 1)))
        got = align_poses(np.asarray(pred)[p], np.asarray(gt)[p], anchor_rotation)
        for k in FIELDS:
            want = base[k][p] if k in ('trans_scaled_error', 'trans_error') else base[k]
            spread[k] = max(spread[k], float(np.abs(np.asarray(got[k]) - want).max()))
    return base, spread


def tolerance(spread):
    """64 x the permutation spread, at least 1e-13: the device decomposes by Jacobi rotations and sums in another order; both are
    backward stable, so their errors scale with the condition number that the spread of the restatement exposes."""
    return {k: max(64.0 * v, 1e-13) for k, v in spread.items()}


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def _rotation(rng, angle=None):
    axis = rng.standard_normal(3)
    axis /= np.linalg.norm(axis)
    angle = rng.uniform(0.3, 2.5) if angle is None else angle
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def _poses(rng, t):
    """(n,4,4) float32 poses at translations t (n,3) with smooth random rotations."""
    n = len(t)
    T = np.tile(np.eye(4), (n, 1, 1))
    R0 = _rotation(rng)
    for i in range(n):
        T[i, :3, :3] = R0 @ _rotation(rng, 0.002 * i)
        T[i, :3, 3] = t[i]
    return T.astype(np.float32)


def make_case(kind, n, seed):
    """(pred, gt) float32 (n,4,4): gt = a similarity of pred's translations plus noise.
    kind 'generic': a 3-D curve; 'planar': pred's z is exactly 0; 'mirrored': gt is a REFLECTION of pred (det(U) det(Vh) < 0 with
    sigma_3 > 0: the best rotation flips the weakest axis)."""
    rng = np.random.default_rng(seed)
    u = np.linspace(0.0, 1.0, n)
    t = np.stack([1.5 * np.cos(2.2 * np.pi * u) + 0.2 * rng.standard_normal(n), 1.1 * np.sin(1.7 * np.pi * u + 0.4) + 0.2 * rng.standard_normal(n),
                  0.6 * u + 0.5 * np.sin(3.1 * np.pi * u) + 0.15 * rng.standard_normal(n)], axis=1) + np.array([0.7, -0.4, 0.3])
    if kind == 'planar':
        t[:, 2] = 0.0
    pred = _poses(rng, t)
    tp = pred[:, :3, 3].astype(np.float64)                        # (as rounded)
    R, s, shift = _rotation(rng), rng.uniform(0.6, 1.8), rng.uniform(-1.0, 1.0, 3)
    if kind == 'mirrored':
        tp = tp * np.array([1.0, 1.0, -1.0])
    tg = s * tp @ R.T + shift + 0.01 * rng.standard_normal((n, 3))
    gt = _poses(rng, tg)
    return pred, gt


# (name, kind, n, seed): the generic lengths ride in ONE launch in the device test (S = 4, n_max = 1000)
CASES = [("generic3", "generic", 3, 11), ("generic65", "generic", 65, 12), ("generic257", "generic", 257, 13), ("generic1000", "generic", 1000, 14),
         ("planar65", "planar", 65, 15), ("mirrored65", "mirrored", 65, 16)]


# ---- the world map -----------------------------------------------------------------------------------------------------------------
def world_points(p, pose, rec=None):
    """p: (Q,3) camera-frame points; pose: (4,4) camera-to-world; rec: dict(s, rot, trans_scaled, rot_reanchor) or None.
    Returns (the world points in float64: R' (s p) + t' with R' = rot_reanchor R, t' = s rot t + trans_scaled -- ``get_dense_pcd`` after
    ``apply_scale``; without ``rec`` R p + t --, and the per-point bound for a float32 evaluation by three fma chains on operands
    rounded once: 8 * 2^-24 * (s |p|_1 + |t'|_inf); |R'| <= 1 entrywise)."""
    p, pose = np.asarray(p, np.float64), np.asarray(pose, np.float64)
    R, t, s = pose[:3, :3], pose[:3, 3], 1.0
    if rec is not None:
        s = float(rec['s'])
        R = np.asarray(rec['rot_reanchor'], np.float64) @ R
        t = s * (np.asarray(rec['rot'], np.float64) @ t) + np.asarray(rec['trans_scaled'], np.float64).reshape(3)
    world = (s * p) @ R.T + t
    bound = 8.0 * 2.0 ** -24 * (abs(s) * np.abs(p).sum(1) + np.abs(t).max())
    return world, bound
