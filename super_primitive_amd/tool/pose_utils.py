"""Trajectory alignment on the device -- the API of the reference's ``tool/pose_utils.py`` (``align``, ``transfer_scale``,
``apply_scale``, ``get_sorted_by_timestamp``) on ``sp_traj_align`` (include/sp_hip.h, csrc/sp_results.hip).

The reference aligns one trajectory with numpy on the host.  Here ``align_trajectories`` aligns S trajectories of different lengths in
ONE launch (one workgroup each, float64 throughout) and leaves the results on the device in one ``SpTrajAlign`` record per trajectory,
which ``odometery.results.keyframe_points`` reads directly; the reference's functions are thin views of that call for S = 1 and return
the reference's dictionary keys as float64 device tensors.  Inputs are device tensors; poses are read as float32."""
from __future__ import annotations

import torch

from .. import _lib

# where the named fields sit in a record, in doubles (struct SpTrajAlign)
_FIELDS = dict(rot=(0, (3, 3)), trans_scaled=(9, (3,)), trans=(12, (3,)), s=(15, ()), rot_reanchor=(16, (3, 3)), ate_scaled=(25, ()),
               ate=(26, ()), dots=(27, ()), norms=(28, ()), sigma=(29, (3,)))


def get_sorted_by_timestamp(pose_dict, return_ids=False):
    """Values of ``{frame id: pose}`` ordered by ``int(frame id)``; with ``return_ids`` also the ids in that order."""
    ids = sorted(pose_dict, key=int)
    poses = [pose_dict[i] for i in ids]
    return (poses, ids) if return_ids else poses


def record_views(record):
    """Named views onto a (S, 32) float64 record tensor (no copies): ``rot`` (S,3,3), ``s`` (S,), ..."""
    S = record.shape[0]
    out = {}
    for name, (at, shape) in _FIELDS.items():
        n = 1
        for d in shape:
            n *= d
        out[name] = record[:, at:at + n].reshape((S,) + shape)
    return out


def align_trajectories(pred, gt, lengths=None, anchor_rotation=False):
    """pred, gt: (S, n_max, 4, 4) camera-to-world poses on the device; ``lengths``: S host integers (default: all ``n_max``), poses at
    and beyond a trajectory's length are padding and never read.  One launch.  Returns dict(record (S, 32) float64 -- the
    ``SpTrajAlign`` records --, the named views onto it (``rot``, ``trans_scaled``, ``trans``, ``s``, ``rot_reanchor``, ``ate_scaled``,
    ``ate``, ``dots``, ``norms``, ``sigma``), ``trans_scaled_error`` / ``trans_error`` (S, n_max), zero in the padding, ``lengths``)."""
    _lib.require_device(pred, gt)
    if pred.dim() != 4 or pred.shape[-2:] != (4, 4) or pred.shape != gt.shape:
        raise ValueError(f"align_trajectories: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must both be (S, n, 4, 4)")
    S, n_max = int(pred.shape[0]), int(pred.shape[1])
    lengths = [n_max] * S if lengths is None else [int(v) for v in lengths]
    if len(lengths) != S:
        raise ValueError(f"align_trajectories: {len(lengths)} lengths for {S} trajectories")
    for n in lengths:
        if n < 3 or n > n_max:
            raise ValueError(f"align_trajectories: a trajectory of {n} poses (3 .. {n_max} are aligned)")
    lib, dev = _lib.load(), pred.device
    p = pred.detach().contiguous().float()
    g = gt.detach().contiguous().float()
    len_d = torch.tensor(lengths, dtype=torch.int32).to(dev)
    record = torch.empty(S, _lib.SP_TRAJ_ALIGN_DOUBLES, dtype=torch.float64, device=dev)
    err_scaled = torch.empty(S, n_max, dtype=torch.float64, device=dev)
    err = torch.empty(S, n_max, dtype=torch.float64, device=dev)
    _lib.check(lib.sp_traj_align(_lib.ptr(p), _lib.ptr(g), _lib.ptr(len_d), S, n_max, 1 if anchor_rotation else 0, _lib.ptr(record),
                                 _lib.ptr(err_scaled), _lib.ptr(err), _lib.stream_ptr()), "sp_traj_align")
    out = dict(record=record, trans_scaled_error=err_scaled, trans_error=err, lengths=lengths, anchor_rotation=bool(anchor_rotation))
    out.update(record_views(record))
    return out


def _as_poses(translations):
    """(3, n) translations -> (1, n, 4, 4) float32 poses with identity rotations."""
    n = translations.shape[1]
    T = torch.eye(4, dtype=torch.float32, device=translations.device).repeat(1, n, 1, 1)
    T[0, :, :3, 3] = translations.t().float()
    return T


def _pose_align(a, model):
    """The reference's ``align`` dictionary from a one-trajectory result and its (3, n) model."""
    rot, s = a['rot'][0], a['s'][0]
    m = model.double()
    return {'rot': rot, 'trans_scaled': a['trans_scaled'][0][:, None], 'trans_scaled_error': a['trans_scaled_error'][0],
            'trans': a['trans'][0][:, None], 'trans_error': a['trans_error'][0], 's': s,
            'model_aligned_scaled': s * (rot @ m) + a['trans_scaled'][0][:, None], 'model_aligned': rot @ m + a['trans'][0][:, None]}


def align(model, data):
    """Horn's closed-form alignment of two (3, n) trajectories: dict(rot (3,3), trans_scaled (3,1), trans_scaled_error (n,), trans
    (3,1), trans_error (n,), s, model_aligned_scaled (3,n), model_aligned (3,n)), float64 on the device."""
    _lib.require_device(model, data)
    if model.dim() != 2 or model.shape[0] != 3 or model.shape != data.shape:
        raise ValueError(f"align: model {tuple(model.shape)} and data {tuple(data.shape)} must both be (3, n)")
    return _pose_align(align_trajectories(_as_poses(model), _as_poses(data)), model)


def _stack(poses):
    return poses if torch.is_tensor(poses) else torch.stack(list(poses))


def transfer_scale(gt_poses, est_poses, anchor_rotation=False):
    """Aligns the estimated poses (list or (n,4,4)) to the ground truth's translations.  Returns (aligned poses (n,4,4) float64:
    translations ``model_aligned_scaled``, rotations ``R_gt[0] R_est[0]^T R`` -- always, as in the reference --, the ``align``
    dictionary, with ``rot_reanchor`` when ``anchor_rotation``)."""
    gt, est = _stack(gt_poses), _stack(est_poses)
    if gt.shape != est.shape or gt.shape[0] == 0:
        raise ValueError(f"transfer_scale: {tuple(est.shape)} estimated poses against {tuple(gt.shape)}")
    a = align_trajectories(est[None], gt[None], anchor_rotation=True)
    pose_align = _pose_align(a, est[:, :3, 3].t())
    out = est.double().clone()
    out[:, :3, 3] = pose_align['model_aligned_scaled'].t()
    out[:, :3, :3] = a['rot_reanchor'][0] @ est[:, :3, :3].double()
    if anchor_rotation:
        pose_align['rot_reanchor'] = a['rot_reanchor'][0]
    return out, pose_align


def apply_scale(T, pose_align):
    """A (4,4) pose in the aligned frame: translation ``s rot t + trans_scaled``, rotation ``rot_reanchor R`` (the identity without
    the key); float64."""
    _lib.require_device(T)
    out = T.double().clone()
    out[:3, 3] = pose_align['s'] * (pose_align['rot'] @ out[:3, 3]) + pose_align['trans_scaled'].reshape(3)
    if 'rot_reanchor' in pose_align:
        out[:3, :3] = pose_align['rot_reanchor'] @ out[:3, :3]
    return out
