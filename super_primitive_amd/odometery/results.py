"""What a sequence reports once it ran: the coloured world map of its keyframes and the trajectory files an evaluator scores.

``keyframe_points``   the reference's viewer rebuilds the point cloud of every window keyframe after each mapping, one ``unproject_kf``
                      per keyframe, down-sampled, scaled by the alignment and transformed by ``apply_scale(T_WC)``
                      (gui/odometery_gui.py:569-575,665-686).  Here keyframes of any sizes, of any number of sequences, go through ONE
                      ``sp_map_points`` launch (include/sp_hip.h) that writes world points, colours, keyframe index and segment id.
``sequence_map``      the map of a ``run_sequence(..., keep_keyframes=True)`` result, aligned against ground-truth poses when given.
``write_tum_format``  the two trajectory files of the reference's ``convert_traj_to_tum.py``."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from .. import _lib
from ..lie.lie_algebra import pose_to_tq
from ..segment_table import table_of
from ..tool import pose_utils

_BLOCK = 256          # rows per workgroup of sp_map_points


def keyframe_points(kfs, klds, poses, stride=1, align=None, align_index=None):
    """kfs: keyframes (``KeyFrame`` with segments); klds: their keypoint log-depths; poses: their camera-to-world poses ((n,4,4) or a
    list); every ``stride``-th table point of each keyframe is reported, i.e. ``unproject_kf(kf, kld)['src_pts'][::stride]`` in the
    world.  ``align``: what ``pose_utils.align_trajectories`` returns (or its (S,32) record tensor); ``align_index``: per keyframe the
    record that moves it into the aligned frame, or -1 for none (default: record 0 for all when ``align`` is given).
    Returns dict(points (Q,3), colours (Q,3) float32, kf_index (Q,), seg_ids (Q,) int32 on the device, offsets: (n+1,) host integers --
    keyframe k owns rows offsets[k] .. offsets[k+1])."""
    n = len(kfs)
    if n == 0 or len(klds) != n or len(poses) != n:
        raise ValueError(f"keyframe_points: {n} keyframes, {len(klds)} log-depth vectors, {len(poses)} poses")
    stride = int(stride)
    if stride < 1:
        raise ValueError(f"keyframe_points: stride {stride}")
    record = align['record'] if isinstance(align, dict) else align
    if align_index is None:
        align_index = [-1 if record is None else 0] * n
    n_align = 0 if record is None else int(record.shape[0])
    if len(align_index) != n or any(not -1 <= int(a) < n_align for a in align_index):
        raise ValueError(f"keyframe_points: align_index {list(align_index)} for {n} keyframes and {n_align} alignment records")
    lib = _lib.load()
    poses_c = (poses if torch.is_tensor(poses) else torch.stack(list(poses))).detach().contiguous().float()
    _lib.require_device(poses_c, record, *[kf.image for kf in kfs], *klds)
    if record is not None and (record.dtype != torch.float64 or record.shape[1:] != (_lib.SP_TRAJ_ALIGN_DOUBLES,) or not record.is_contiguous()):
        raise ValueError("keyframe_points: align must be the (S, 32) float64 records of align_trajectories")
    recs = (_lib.SpMapKeyframe * n)()
    keep = [poses_c]                                       # the tensors the records point at, alive until the launch is queued
    offsets = np.zeros(n + 1, dtype=np.int64)
    block = 0
    for k, (kf, kld) in enumerate(zip(kfs, klds)):
        tab = table_of(kf)                                 # (raises ValueError for a keyframe without segment pixels)
        image = kf.image[:3].detach().contiguous().float()
        if tuple(image.shape) != (3, tab.H, tab.W):
            raise ValueError(f"keyframe_points: keyframe {k}: image {tuple(image.shape)} against segments of {tab.H}x{tab.W}")
        kld_c, K_c = kld.detach().contiguous().float(), kf.K.detach().contiguous().float()
        if kld_c.numel() != tab.N or K_c.numel() != 9 or poses_c[k].numel() != 16:
            raise ValueError(f"keyframe_points: keyframe {k}: {kld_c.numel()} log-depths for {tab.N} segments, K of {K_c.numel()}, pose of {poses_c[k].numel()}")
        keep += [tab, image, kld_c, K_c]
        r = recs[k]
        r.pix, r.baseL, r.seg_off, r.kp_L = tab.pix.data_ptr(), tab.baseL.data_ptr(), tab.seg_off.data_ptr(), tab.kp_L.data_ptr()
        r.kld, r.image, r.K, r.pose = kld_c.data_ptr(), image.data_ptr(), K_c.data_ptr(), poses_c[k].data_ptr()
        r.N, r.P, r.H, r.W = tab.N, tab.P, tab.H, tab.W
        q = (tab.P + stride - 1) // stride
        r.out_offset, r.align, r.first_block = int(offsets[k]), int(align_index[k]), block
        offsets[k + 1] = offsets[k] + q
        block += (q + _BLOCK - 1) // _BLOCK
    total = int(offsets[-1])
    dev = poses_c.device
    recs_d = torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(dev)
    out = dict(points=torch.empty(total, 3, dtype=torch.float32, device=dev), colours=torch.empty(total, 3, dtype=torch.float32, device=dev),
               kf_index=torch.empty(total, dtype=torch.int32, device=dev), seg_ids=torch.empty(total, dtype=torch.int32, device=dev))
    _lib.check(lib.sp_map_points(_lib.ptr(recs_d), n, block, stride, _lib.ptr(record), n_align, _lib.ptr(out['points']), _lib.ptr(out['colours']),
                                 _lib.ptr(out['kf_index']), _lib.ptr(out['seg_ids']), total, _lib.stream_ptr()), "sp_map_points")
    out['offsets'] = offsets
    return out


def sequence_map(result, stride, gt_poses=None, anchor_rotation=True):
    """The world map of every keyframe a sequence created: ``result`` is what ``run_sequence`` / ``run_sequences`` returned with
    ``keep_keyframes=True``; the keyframes appear in frame order, each at its archived pose and log-depths.  ``gt_poses``: ground-truth
    camera-to-world poses indexed by frame id ((n_frames,4,4), a list or a dict): the keyframe trajectory is aligned against them at
    its own ids (``transfer_scale``'s alignment) and the map is moved into the ground truth's frame.
    Returns ``keyframe_points``' dict plus ``ids`` (frame id per keyframe) and, with ``gt_poses``, ``align`` (what
    ``align_trajectories`` returns, one trajectory), ``traj_ids``, ``ate_scaled`` and ``ate`` (0-dim device tensors)."""
    archive = result['kf_archive']
    ids = sorted(archive)
    if any(archive[i]['kf'] is None for i in ids):
        raise ValueError("sequence_map: the result holds no keyframes (run with keep_keyframes=True)")
    extra = {}
    align = None
    if gt_poses is not None:
        traj, traj_ids = pose_utils.get_sorted_by_timestamp(result['kf_trajectory'], return_ids=True)
        pred = torch.stack(traj)
        gt = torch.stack([torch.as_tensor(gt_poses[i]).to(pred.device) for i in traj_ids])
        align = pose_utils.align_trajectories(pred[None], gt[None], anchor_rotation=anchor_rotation)
        extra = dict(align=align, traj_ids=traj_ids, ate_scaled=align['ate_scaled'][0], ate=align['ate'][0])
    out = keyframe_points([archive[i]['kf'] for i in ids], [archive[i]['kld'] for i in ids], [archive[i]['pose'] for i in ids],
                          stride=stride, align=align)
    out['ids'] = ids
    out.update(extra)
    return out


def write_tum_format(timestamps, pred_poses, gt_poses, out_dir):
    """``timestamp tx ty tz qx qy qz qw`` per line into ``out_dir/converted_tum_traj.txt`` (pred_poses) and
    ``out_dir/converted_gt_tum_traj.txt`` (gt_poses); poses are (n,4,4) tensors or arrays, or lists of (4,4).  Device poses come to the
    host in one copy.  Returns the two paths."""
    def host(poses):
        if torch.is_tensor(poses) or (len(poses) and torch.is_tensor(poses[0])):
            poses = poses if torch.is_tensor(poses) else torch.stack(list(poses))
            return poses.detach().double()
        return torch.from_numpy(np.asarray(poses, dtype=np.float64))
    pred, gt = host(pred_poses), host(gt_poses)
    if not (len(timestamps) == pred.shape[0] == gt.shape[0]) or pred.shape[1:] != (4, 4) or gt.shape[1:] != (4, 4):
        raise ValueError(f"write_tum_format: {len(timestamps)} timestamps, poses {tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.device == gt.device:
        both = torch.cat((pred, gt)).cpu().numpy()                     # the one device-to-host copy
    else:
        both = np.concatenate((pred.cpu().numpy(), gt.cpu().numpy()))
    tq = pose_to_tq(both)
    path = Path(out_dir)
    path.mkdir(parents=True, exist_ok=True)
    files = (path / 'converted_tum_traj.txt', path / 'converted_gt_tum_traj.txt')
    n = len(timestamps)
    for file, rows in zip(files, (tq[:n], tq[n:])):
        with open(file, 'w') as f:
            for ts, p in zip(timestamps, rows):
                f.write(f'{ts} {p[0]} {p[1]} {p[2]} {p[3]} {p[4]} {p[5]} {p[6]}\n')
    return files
