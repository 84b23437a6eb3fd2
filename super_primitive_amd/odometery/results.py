"""What a sequence reports once it ran: the coloured world map of its keyframes and the trajectory files an evaluator scores.

``keyframe_points``   the reference's viewer rebuilds the point cloud of every window keyframe after each mapping, one ``unproject_kf``
                      per keyframe, down-sampled, scaled by the alignment and transformed by ``apply_scale(T_WC)``
                      (gui/odometery_gui.py:569-575,665-686).  Here keyframes of any sizes, of any number of sequences, go through ONE
                      ``sp_map_points`` launch (include/sp_hip.h) that writes world points, colours, keyframe index and segment id.
``sequence_map``      the map of a ``run_sequence(..., keep_keyframes=True)`` result, aligned against ground-truth poses when given.
``render_map``        the map seen from V cameras (image, depth buffer, winning point per pixel), ONE ``sp_render_views`` launch.
``score_map``         the map's depth buffer in the ground-truth views against ground-truth depth: ``sp_depth_metrics`` and the coverage.
``point_radii``       the size of the source pixels every map point stands for: the footprints that ``render_map`` / ``score_map`` /
                      ``score_map_images`` splat through the depth buffer (``sp_render_splats``), so a sparse map has no holes.
``score_map_images``  the map's rendered views against real images: PSNR, L1 and coverage from ``sp_image_metrics``' integer sums.
                      With ``normals=True`` -- on a map made with ``normals=True``: one ``sp_map_normals`` launch over the same records --
                      the three render every point as an oriented surfel (``sp_render_surfels``): slanted surfaces at their true depth.
``map_consistency``   every map point against V depth images -- the other keyframes' own, or ground truth: per point the views it
                      agrees with, floats in front of, is hidden behind (ONE ``sp_map_consistency`` launch); ``sequence_consistency`` is
                      the self-check of a sequence's map without ground truth, ``segment_consistency`` the verdict per (keyframe,
                      segment), ``filter_map`` the map with the unconfirmed points taken out.
``fuse_map``          the map as a map: one averaged point per occupied voxel (ONE ``sp_map_fuse`` call), a world dict every function
                      above accepts; ``pool_map`` sums per-input-point integers (consistency counts) per fused point.
``map_distance``      the map against a reference CLOUD (lifted ground-truth depths) in 3D: per point the nearest point of the other cloud
                      within a radius, both ways (``sp_cloud_grid_build`` / ``sp_cloud_grid_nearest``), and ``cloud_metrics`` of the two
                      distance vectors: accuracy, completion, precision, recall, F-score; ``map_neighbours`` is the map against itself:
                      its spacing and the neighbour count a radius outlier filter keeps points by.
``register_map``      the map moved onto a reference cloud by ICP on the device before it is scored (``sp_cloud_register``): the 3D scores no
                      longer hang on a similarity fitted to a handful of camera centres; ``transform_map`` applies any similarity to a map.
``estimate_normals``  normals for a cloud that has none -- lifted ground truth, a fused map, a scan --, from the k nearest points of every
                      point (``sp_cloud_grid_knn`` / ``sp_cloud_normals``): ``register_map`` then reaches its ``'plane'`` residual and
                      ``write_ply`` exports ``nx ny nz``; ``statistical_outliers`` is the mean distance to the k nearest against the
                      cloud's mean and deviation, ``select_map`` the map reduced to the rows a mask keeps.
``write_tum_format``  the two trajectory files of the reference's ``convert_traj_to_tum.py``.
``fuse_tsdf``         depth images fused into one dense signed-distance volume (``tsdf_volume``; ONE ``sp_tsdf_integrate`` launch):
                      the average of what every view saw; ``sequence_tsdf`` fuses a sequence's own keyframes, ``extract_mesh`` cuts the
                      zero level set into an indexed triangle mesh (``sp_tsdf_mesh``) whose vertices are a cloud every function above takes.
``render_surface``    the fused surface seen from V cameras, one ray per pixel through the volume (ONE ``sp_tsdf_raycast`` launch): depth at
                      the zero crossing, normals from the field's gradient, interpolated colour, the cell behind the surface;
                      ``score_surface`` / ``score_surface_images`` score those views against ground-truth depth and real images, as
                      ``score_map`` / ``score_map_images`` score the points (the scoring tails are shared).
``sample_mesh``       a mesh -- ``extract_mesh``'s, or a ground-truth model's -- as a surface: an area-uniform, seeded cloud with exact
                      normals (``sp_mesh_faces`` / ``sp_mesh_sample``) that every function above takes; ``mesh_faces`` is the record per
                      face, ``clean_mesh`` drops degenerate triangles, ``mesh_normals`` gives area-weighted vertex normals and
                      ``mesh_distance`` scores surface against surface, both meshes sampled at one density.
``render_mesh``       a mesh seen from V cameras, rasterised through the depth buffer (ONE ``sp_mesh_render`` call): depth, the winning
                      face and its normal, interpolated colour -- ground-truth depth images from a ground-truth model; ``score_mesh`` /
                      ``score_mesh_images`` score those views as ``score_surface`` / ``score_surface_images`` score the volume's,
                      ``visible_faces`` counts the pixels and views every face wins, ``cull_mesh`` keeps what the cameras saw.
``write_ply``         the map's points, normals (when it has them) and 8-bit colours as a binary PLY file; a mesh's faces too;
                      ``read_ply`` is its inverse, for binary and ASCII files of triangles."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from .. import _lib
from ..lie.lie_algebra import pose_to_tq
from ..tool import pose_utils


def keyframe_points(kfs, klds, poses, stride=1, align=None, align_index=None, normals=False):
    """kfs: keyframes (``KeyFrame`` with segments); klds: their keypoint log-depths; poses: their camera-to-world poses ((n,4,4) or a
    list); every ``stride``-th table point of each keyframe is reported, i.e. ``unproject_kf(kf, kld)['src_pts'][::stride]`` in the
    world.  ``align``: what ``pose_utils.align_trajectories`` returns (or its (S,32) record tensor); ``align_index``: per keyframe the
    record that moves it into the aligned frame, or -1 for none (default: record 0 for all when ``align`` is given).
    Returns dict(points (Q,3), colours (Q,3) float32, kf_index (Q,), seg_ids (Q,) int32 on the device, offsets: (n+1,) host integers --
    keyframe k owns rows offsets[k] .. offsets[k+1]).  ``normals=True``: also ``normals`` (Q,3) float32, the unit surface normal of
    every row in the world, facing its keyframe's camera, (0, 0, 0) where the table gives none -- a second launch (``sp_map_normals``)
    over the same records."""
    from ..tool import viz
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
    recs_d, keep, offsets, blocks = viz.keyframe_records("keyframe_points", kfs, klds, stride, poses_c, align_index)    # (keep: alive until the launch)
    total, dev = offsets[-1], poses_c.device
    out = dict(points=torch.empty(total, 3, dtype=torch.float32, device=dev), colours=torch.empty(total, 3, dtype=torch.float32, device=dev),
               kf_index=torch.empty(total, dtype=torch.int32, device=dev), seg_ids=torch.empty(total, dtype=torch.int32, device=dev))
    _lib.check(lib.sp_map_points(_lib.ptr(recs_d), n, blocks, stride, _lib.ptr(record), n_align, _lib.ptr(out['points']), _lib.ptr(out['colours']),
                                 _lib.ptr(out['kf_index']), _lib.ptr(out['seg_ids']), total, _lib.stream_ptr()), "sp_map_points")
    if normals:
        out['normals'] = viz.keyframe_normals(recs_d, n, blocks, stride, total, record)
    out['offsets'] = np.asarray(offsets, dtype=np.int64)
    return out


def sequence_map(result, stride, gt_poses=None, anchor_rotation=True, normals=False):
    """The world map of every keyframe a sequence created: ``result`` is what ``run_sequence`` / ``run_sequences`` returned with
    ``keep_keyframes=True``; the keyframes appear in frame order, each at its archived pose and log-depths.  ``gt_poses``: ground-truth
    camera-to-world poses indexed by frame id ((n_frames,4,4), a list or a dict): the keyframe trajectory is aligned against them at
    its own ids (``transfer_scale``'s alignment) and the map is moved into the ground truth's frame.
    Returns ``keyframe_points``' dict plus ``ids`` (frame id per keyframe) and, with ``gt_poses``, ``align`` (what
    ``align_trajectories`` returns, one trajectory), ``traj_ids``, ``ate_scaled`` and ``ate`` (0-dim device tensors).  ``normals``: as in
    ``keyframe_points``."""
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
                          stride=stride, align=align, normals=normals)
    out['ids'] = ids
    out.update(extra)
    return out


def _view_cameras(Ks, poses, what):
    """(V,3,3) cameras and (V,4,4) poses from tensors or lists; ``Ks`` may be one (3,3) for all."""
    poses = poses if torch.is_tensor(poses) else torch.stack(list(poses))
    Ks = Ks if torch.is_tensor(Ks) else torch.stack(list(Ks))
    if poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4) or poses.shape[0] == 0:
        raise ValueError(f"{what}: poses must be (V,4,4), got {tuple(poses.shape)}")
    return Ks, poses


def _map_poses(world, result):
    """(n,4,4) float64: the archive poses of ``world['ids']`` in the map's frame -- moved by ``pose_utils.apply_scale`` when ``world``
    carries ``align``."""
    archive = result['kf_archive']
    dev = world['points'].device
    a = world.get('align')
    poses = []
    for i in world['ids']:
        T = archive[i]['pose'].detach().to(dev)
        if a is not None:
            T = pose_utils.apply_scale(T, dict(s=a['s'][0], rot=a['rot'][0], trans_scaled=a['trans_scaled'][0], rot_reanchor=a['rot_reanchor'][0]))
        poses.append(T.double())
    return torch.stack(poses)


def point_radii(world, result, footprint=1.0):
    """The footprint of every map point in world units, for ``render_map`` / ``score_map`` / ``score_map_images`` (``radii=``): a point
    stands for ``footprint`` source pixels of its keyframe, so its half side is ``radius_i = footprint / (2 fx_k) * a_k . (p_i - c_k)``
    with ``k = world['kf_index'][i]`` and ``c_k``, ``a_k`` the centre and the optical axis (third rotation column) of keyframe k's pose
    in the map's frame: the archive pose of ``result`` (what ``run_sequence(..., keep_keyframes=True)`` returned), moved by
    ``pose_utils.apply_scale`` when ``world`` carries ``align``.  With an alignment ``a . (p - c) = s z_cam``: the radius scales with the
    map.  ``stride`` of ``sequence_map`` counts points along TABLE order (segment after segment, row-major within one), not along both
    image axes, so the footprint that closes a stride-4 map is the caller's choice (2 if the points were spread evenly, up to 4 along
    a row).  Returns (Q,) float32 on the device; a handful of torch ops, no host read."""
    archive = result['kf_archive']
    ids = world['ids']
    if any(archive[i]['kf'] is None for i in ids):
        raise ValueError("point_radii: the result holds no keyframes (run with keep_keyframes=True)")
    if not float(footprint) >= 0.0:
        raise ValueError(f"point_radii: footprint {footprint}")
    points = world['points']
    _lib.require_device(points, world['kf_index'])
    poses = _map_poses(world, result)
    fx = torch.stack([archive[i]['kf'].K.detach().reshape(-1)[0].to(points.device) for i in ids]).double()
    k = world['kf_index'].long()
    depth = ((points.double() - poses[:, :3, 3][k]) * poses[:, :3, 2][k]).sum(dim=1)
    return ((float(footprint) / (2.0 * fx))[k] * depth).float()


def _surfel_normals(world, normals, radii, what):
    """``world['normals']`` for a render with ``normals=True`` (``ValueError`` if the world has none or ``radii`` is missing), else None."""
    if not normals:
        return None
    if world.get('normals') is None or radii is None:
        raise ValueError(f"{what}: normals=True needs world['normals'] (keyframe_points / sequence_map with normals=True) and radii")
    return world['normals']


def render_map(world, Ks, poses, size, depth_buffer=True, radii=None, max_px=8, normals=False, cull=False):
    """The map seen from V cameras in ONE ``sp_render_views`` launch (``tool.viz.render_views``): ``world`` is what ``keyframe_points`` or
    ``sequence_map`` returned (its ``points`` and ``colours``), ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4) camera-to-world in the map's
    frame, ``size`` = (H, W).  ``depth_buffer=True``: the nearest point in front of the camera wins a pixel; False: the reference's
    ``render_pcd`` (the highest index wins, nothing is tested against z).  ``radii`` ((Q,) float32, ``point_radii``): every point is a
    square footprint of that half side, at most ``max_px`` pixels to either side (ONE ``sp_render_splats`` launch): a map sparser than
    the view leaves no holes and the nearer surface hides the farther one.  ``normals=True`` (with ``radii``; ``world['normals']``
    must exist): every point is an oriented surfel (ONE ``sp_render_surfels`` launch), the depth of each covered pixel taken on its
    tangent plane; ``cull=True`` drops surfels seen from behind.
    Returns dict(image (V,H,W,3) uint8, depth (V,H,W) float32 -- 0 where nothing landed --, index (V,H,W) int32 -- the winning row of
    ``world['points']``, -1 where nothing landed).  Per-pixel keyframe and segment maps follow from it:
    ``torch.where(index >= 0, world['kf_index'][index.clamp(min=0).long()], -1)``, and the same with ``world['seg_ids']``.
    No synchronisation."""
    from ..tool import viz
    Ks, poses = _view_cameras(Ks, poses, "render_map")
    H, W = size
    return viz.render_views(world['points'], world['colours'], Ks, poses, H, W, depth_buffer=depth_buffer, radii=radii, max_px=max_px,
                            normals=_surfel_normals(world, normals, radii, "render_map"), cull=cull)


def _target_images(images, poses, what):
    """(H, W) of ``images``, which must be float32 (V,3,H,W) for the V ``poses``."""
    if not torch.is_tensor(images) or images.dim() != 4 or images.shape[0] != poses.shape[0] or images.shape[1] != 3 or images.dtype != torch.float32:
        raise ValueError(f"{what}: images must be float32 (V,3,H,W) for {poses.shape[0]} views, got "
                         f"{tuple(images.shape) if torch.is_tensor(images) else type(images).__name__}")
    return int(images.shape[2]), int(images.shape[3])


def _image_scores(rendered, images, index):
    """The tail of ``score_map_images`` / ``score_surface_images``: ONE ``sp_image_metrics`` launch over the pixels with ``index >= 0`` and
    the figures from its integer sums."""
    from ..tool import viz
    H, W = int(images.shape[2]), int(images.shape[3])
    sums = viz.image_metrics(rendered, images, index)
    n3, s1, s2 = 3.0 * sums[:, 0].double(), sums[:, 1].double(), sums[:, 2].double()
    return dict(sums=sums, psnr=10.0 * torch.log10(255.0 ** 2 * n3 / s2), l1=s1 / n3, coverage=sums[:, 0].double() / float(H * W))


def score_map_images(world, images, Ks, poses, radii=None, max_px=8, normals=False, cull=False):
    """The map's rendered views against real images: ``images`` (V,3,H,W) float32 in 0..1, ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4)
    camera-to-world in the map's frame; ``radii`` / ``max_px`` / ``normals`` / ``cull`` as in ``render_map``.  One render launch (depth buffer) plus ONE
    ``sp_image_metrics`` launch; only pixels something landed on are compared, at 8 bits per channel.
    Returns dict(sums (V,3) int64 -- n, sum |a - b|, sum (a - b)^2 over the compared pixels' three channels --, psnr (V,) float64 =
    10 log10(255^2 3n / sum d^2) (NaN for n = 0, inf for identical pixels), l1 (V,) float64 in 0..255 = sum |a - b| / 3n (NaN for
    n = 0), coverage (V,) float64 = n / (H W)).  No synchronisation."""
    from ..tool import viz
    Ks, poses = _view_cameras(Ks, poses, "score_map_images")
    H, W = _target_images(images, poses, "score_map_images")
    _lib.require_device(images, world['points'])
    out = viz.render_views(world['points'], world['colours'], Ks, poses, H, W, depth_buffer=True, depth=False, radii=radii, max_px=max_px,
                           normals=_surfel_normals(world, normals, radii, "score_map_images"), cull=cull)
    return _image_scores(out['image'], images, out['index'])


def _target_depths(gt_depths, gt_poses, min_depth, max_depth, what):
    """(V, H, W) of ``gt_depths``, which must be float32 (V,H,W) for the V ``gt_poses``; the depth range must not be empty."""
    if not torch.is_tensor(gt_depths) or gt_depths.dim() != 3 or gt_depths.shape[0] != gt_poses.shape[0] or gt_depths.dtype != torch.float32:
        raise ValueError(f"{what}: gt_depths must be float32 (V,H,W) for {gt_poses.shape[0]} views, got "
                         f"{tuple(gt_depths.shape) if torch.is_tensor(gt_depths) else type(gt_depths).__name__}")
    if not float(min_depth) <= float(max_depth):
        raise ValueError(f"{what}: depth range {min_depth} .. {max_depth}")
    return tuple(int(n) for n in gt_depths.shape)


def _depth_scores(depth, landed, gt_depths, min_depth, max_depth):
    """The tail of ``score_map`` / ``score_surface``: ``depth`` (V,H,W) scored against ``gt_depths`` on the pixels where something ``landed``
    and ``min_depth <= gt <= max_depth``: ONE ``sp_depth_metrics`` call, and the coverage."""
    from ..depth_completion import void
    in_range = (gt_depths >= min_depth) & (gt_depths <= max_depth)
    scored = in_range & landed
    metrics = void.depth_metrics(depth, gt_depths, scored)
    coverage = scored.sum(dim=(1, 2)).double() / in_range.sum(dim=(1, 2)).double()
    return dict(metrics=metrics, columns=void._COLUMNS, coverage=coverage)


def score_map(world, gt_depths, Ks, gt_poses, min_depth=0.2, max_depth=5.0, size=None, radii=None, max_px=8, normals=False, cull=False):
    """The map against ground-truth depth images: its depth buffer is rendered into each of the V ground-truth views (``render_map``'s
    launch, depth only) and scored where it landed.  ``gt_depths`` (V,H,W) float32, ``Ks`` (V,3,3) or (3,3), ``gt_poses`` (V,4,4)
    camera-to-world; the map should already be in the ground truth's frame, as ``sequence_map(gt_poses=...)`` delivers it.
    A pixel is scored iff the rendered depth is > 0 and ``min_depth <= gt <= max_depth``.  ONE ``sp_depth_metrics`` call for all views.
    Returns dict(metrics (V,12) float64 on the device, columns: the names of its columns (``depth_completion.void``: n, rmse, mae, absrel
    in mm, inv_rmse, inv_mae, inv_absrel in 1/km, delta105, delta110, delta1, delta2, delta3), coverage (V,) float64 = scored pixels /
    pixels with ``min_depth <= gt <= max_depth`` (NaN for a view without any)).  ``size``: an (H, W) the depths must have, if given.
    ``radii`` / ``max_px``: the footprints of ``render_map``, so that a sparse map is scored on every pixel its surfaces cover;
    ``normals`` / ``cull``: its oriented surfels, so that the score carries no error of a flat splat on a slanted surface.
    No synchronisation."""
    from ..tool import viz
    Ks, gt_poses = _view_cameras(Ks, gt_poses, "score_map")
    V, H, W = _target_depths(gt_depths, gt_poses, min_depth, max_depth, "score_map")
    if size is not None and tuple(int(s) for s in size) != (H, W):
        raise ValueError(f"score_map: size {tuple(size)} against ground-truth depths of {H}x{W}")
    _lib.require_device(gt_depths, world['points'])
    depth = viz.render_views(world['points'], None, Ks, gt_poses, H, W, depth_buffer=True, image=False, index=False, radii=radii,
                             max_px=max_px, normals=_surfel_normals(world, normals, radii, "score_map"), cull=cull)['depth']
    return _depth_scores(depth, depth > 0, gt_depths, min_depth, max_depth)


def map_consistency(world, depths, Ks, poses, view_kf=None, tol=0.05, window=1):
    """Every map point against V depth images in ONE ``sp_map_consistency`` launch (``tool.viz.map_consistency``; include/sp_hip.h has
    the rule): ``depths`` (V,H,W) float32 is what each view claims to see -- the keyframes' own depth images (``sequence_consistency``)
    or ground truth, for per-point accuracy --, ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4) camera-to-world in the map's frame.
    ``view_kf`` ((V,) integers or None): the keyframe (row of ``world['kf_index']``) each view belongs to; a point is never tested
    against a view of its own keyframe.  Returns dict(counts (Q,3) int32 -- the views a point agrees with / floats in front of (the view
    looks straight through it) / is hidden behind --, agree, in_front, behind: its columns, seen (Q,) int32: their sum).
    No synchronisation."""
    from ..tool import viz
    Ks, poses = _view_cameras(Ks, poses, "map_consistency")
    V = int(poses.shape[0])
    if not torch.is_tensor(depths) or depths.dim() != 3 or depths.shape[0] != V or depths.dtype != torch.float32:
        raise ValueError(f"map_consistency: depths must be float32 (V,H,W) for {V} views, got "
                         f"{tuple(depths.shape) if torch.is_tensor(depths) else type(depths).__name__}")
    owner = view_owner = None
    if view_kf is not None:
        view_owner = torch.as_tensor(view_kf)
        if view_owner.is_floating_point() or tuple(view_owner.shape) != (V,):
            raise ValueError(f"map_consistency: view_kf must be {V} integers, got {view_owner.dtype} {tuple(view_owner.shape)}")
        view_owner = view_owner.to(device=world['points'].device, dtype=torch.int32)
        owner = world['kf_index']
    counts = viz.map_consistency(world['points'], Ks, poses, depths, owner=owner, view_owner=view_owner, tol=tol, window=window)
    return dict(counts=counts, agree=counts[:, 0], in_front=counts[:, 1], behind=counts[:, 2], seen=counts.sum(dim=1, dtype=torch.int32))


def sequence_consistency(world, result, tol=0.05, window=1):
    """The map's self-check, without ground truth: every point of ``world`` (``sequence_map`` of ``result``) against the depth image each
    OTHER keyframe claims to see (``tool.viz.keyframe_depths`` on the archive, in ``world['ids']`` order; multiplied by the alignment
    scale when ``world`` carries ``align``: the world points are scaled, the tables are not), through the archive poses in the map's
    frame (``point_radii``'s).  Returns ``map_consistency``'s dict plus ``depths`` (n,H,W) float32 and ``seg_maps`` (n,H,W) int32.
    No synchronisation beyond the keyframes' table builds."""
    views = _sequence_views(world, result, "sequence_consistency")
    out = map_consistency(world, views['depths'], views['Ks'], views['poses'], view_kf=torch.arange(len(world['ids']), dtype=torch.int32),
                          tol=tol, window=window)
    out.update(depths=views['depths'], seg_maps=views['seg_maps'])
    return out


def _sequence_views(world, result, what):
    """What the keyframes of ``world`` (``sequence_map`` of ``result``) claim to see, in the map's frame: ``dict(depths (n,H,W) float32 --
    ``tool.viz.keyframe_depths`` on the archive, in ``world['ids']`` order, multiplied by the alignment scale when ``world`` carries
    ``align`` --, seg_maps (n,H,W) int32, Ks (n,3,3), poses (n,4,4) float64 -- ``_map_poses``)``: the views ``sequence_consistency`` tests the
    map against and ``sequence_tsdf`` fuses."""
    from ..tool import viz
    archive = result['kf_archive']
    ids = world['ids']
    if any(archive[i]['kf'] is None for i in ids):
        raise ValueError(f"{what}: the result holds no keyframes (run with keep_keyframes=True)")
    _lib.require_device(world['points'], world['kf_index'])
    own = viz.keyframe_depths([archive[i]['kf'] for i in ids], [archive[i]['kld'] for i in ids])
    depths = own['depth']
    a = world.get('align')
    if a is not None:
        depths = depths * a['s'][0].to(torch.float32)
    dev = depths.device
    Ks = torch.stack([archive[i]['kf'].K.detach().reshape(3, 3).to(dev) for i in ids])
    return dict(depths=depths, seg_maps=own['seg'], Ks=Ks, poses=_map_poses(world, result))


def segment_consistency(world, consistency, n_segments=None):
    """A verdict per (keyframe, segment) from ``map_consistency``'s per-point counts: (n_kf, N_max, 5) int64 on the points' device --
    points; points seen at least once; points with ``agree >= 1``; points with ``in_front >= 1`` and ``agree == 0`` (some view looks
    through them and none confirms them); the sum of ``agree``.  Integer sums per integer key (one ``index_add_``): exact, whatever the
    order.  ``n_segments``: N_max; without it the largest segment id is read from the device (the one host read).  Points whose
    segment id lies outside 0 .. N_max - 1 are counted nowhere."""
    kf, seg = world['kf_index'].long(), world['seg_ids'].long()
    counts = consistency['counts']
    if counts.dim() != 2 or counts.shape != (kf.shape[0], 3) or seg.shape != kf.shape:
        raise ValueError(f"segment_consistency: counts {tuple(counts.shape)} for {kf.shape[0]} points")
    n_kf = len(world['offsets']) - 1
    n_max = int(n_segments) if n_segments is not None else int(seg.max()) + 1
    if n_max < 1:
        raise ValueError(f"segment_consistency: {n_max} segments")
    agree, front = counts[:, 0].long(), counts[:, 1].long()
    seen = counts.sum(dim=1) > 0
    values = torch.stack((torch.ones_like(agree), seen.long(), (agree >= 1).long(), ((front >= 1) & (agree == 0)).long(), agree), dim=1)
    inside = (seg >= 0) & (seg < n_max) & (kf >= 0) & (kf < n_kf)
    key = torch.where(inside, kf * n_max + seg, torch.full_like(kf, n_kf * n_max))     # (one row beyond the table takes the rest)
    out = torch.zeros(n_kf * n_max + 1, 5, dtype=torch.int64, device=kf.device).index_add_(0, key, values)
    return out[:-1].reshape(n_kf, n_max, 5)


_PER_POINT = ('points', 'colours', 'kf_index', 'seg_ids')
_NORMAL_SCALE = 2.0 ** 20          # fuse_map: member normals are summed as int32 round(n * 2^20)


def _check_world(world, what):
    """``filter_map``'s conditions on a world dict: the four per-point tensors, of one length, and offsets ending at it."""
    missing = [k for k in _PER_POINT + ('offsets',) if world.get(k) is None]
    if missing or not all(torch.is_tensor(world[k]) for k in _PER_POINT):
        raise ValueError(f"{what}: world needs tensors {_PER_POINT} and offsets; missing or not tensors: "
                         f"{missing or [k for k in _PER_POINT if not torch.is_tensor(world[k])]}")
    Q = int(world['points'].shape[0])
    if any(int(world[k].shape[0]) != Q for k in _PER_POINT) or int(np.asarray(world['offsets'])[-1]) != Q:
        raise ValueError(f"{what}: {[(k, int(world[k].shape[0])) for k in _PER_POINT]} rows and offsets ending at "
                         f"{int(np.asarray(world['offsets'])[-1])} for {Q} points")
    nrm = world.get('normals')
    if nrm is not None and (not torch.is_tensor(nrm) or nrm.dtype != torch.float32 or tuple(nrm.shape) != (Q, 3)):
        raise ValueError(f"{what}: world['normals'] must be a float32 tensor ({Q},3)")
    return Q


def filter_map(world, consistency, min_agree=1, max_in_front=None):
    """The map a user would export: the rows of ``world`` with ``agree >= min_agree`` -- and ``in_front <= max_in_front`` if given --,
    in their order.  Returns a new dict: ``points``, ``colours``, ``kf_index``, ``seg_ids`` (and ``normals``, if the world has them)
    compacted, ``offsets`` recomputed (host
    integers, as ``keyframe_points`` returns them), ``kept`` (int64, on the device: the surviving rows of ``world``); every other entry
    (``ids``, ``align``, the ATE fields) is carried over.  ``world`` must hold all four per-point tensors, of one length, and ``offsets``
    ending at that length (``ValueError`` otherwise).  Sizing the output takes ONE host read -- the new offsets, n_kf + 1 integers;
    everything before it is asynchronous, and the compaction after it (a scatter of the row numbers to their ranks) reads nothing
    back."""
    counts = consistency['counts']
    Q = _check_world(world, "filter_map")
    if counts.dim() != 2 or tuple(counts.shape) != (Q, 3):
        raise ValueError(f"filter_map: counts {tuple(counts.shape)} for {Q} points")
    keep = counts[:, 0] >= int(min_agree)
    if max_in_front is not None:
        keep = keep & (counts[:, 1] <= int(max_in_front))
    return _select_rows(world, keep, Q)


def _select_rows(world, keep, Q):
    """The rows of ``world`` (validated, Q rows) where ``keep`` (Q,) bool holds, in their order: the compaction of ``filter_map`` and
    ``select_map``.  ONE host read, the new offsets."""
    dev = keep.device
    rank = torch.cumsum(keep.long(), dim=0)                                            # inclusive: rank[i] - 1 is row i's new place
    before = torch.cat((rank.new_zeros(1), rank))                                      # before[o] = kept rows among the first o
    old = torch.as_tensor(np.asarray(world['offsets'], dtype=np.int64)).to(dev)
    offsets = before[old].cpu().numpy()                                                # the one host read
    total = int(offsets[-1])
    dest = torch.where(keep, rank - 1, torch.full_like(rank, total))                   # (dropped rows all go to one spare slot)
    kept = torch.empty(total + 1, dtype=torch.int64, device=dev).scatter_(0, dest, torch.arange(Q, dtype=torch.int64, device=dev))[:total]
    out = {k: v for k, v in world.items() if k not in _PER_POINT and k != 'offsets'}
    for k in _PER_POINT + (('normals',) if world.get('normals') is not None else ()):
        out[k] = world[k][kept]
    out['offsets'] = offsets
    out['kept'] = kept
    return out


def select_map(world, keep):
    """``world`` reduced to the rows where ``keep`` (Q,) bool holds -- ``statistical_outliers(...)['keep']``, ``map_neighbours(...)
    ['count'] >= n``, any mask of the caller's --, in their order: what ``filter_map`` returns for its own mask (the same code): the
    per-point tensors (and ``normals``, if the world has them) compacted, ``offsets`` recomputed, ``kept`` the surviving rows, every
    other entry carried over.  ``world`` is validated as ``filter_map`` does.  ONE host read, the new offsets."""
    Q = _check_world(world, "select_map")
    if not torch.is_tensor(keep) or keep.dtype != torch.bool or tuple(keep.shape) != (Q,):
        raise ValueError(f"select_map: keep must be a bool tensor ({Q},), got "
                         f"{(keep.dtype, tuple(keep.shape)) if torch.is_tensor(keep) else type(keep).__name__}")
    return _select_rows(world, keep, Q)


def fuse_map(world, voxel, origin=None):
    """The map as a map: every keyframe contributes its own copy of each surface it sees, so ``world`` grows with the number of
    keyframes; here the points of one voxel (side ``voxel``, grid through ``origin``, default 0, 0, 0) become ONE point, their mean
    position and mean colour (ONE ``sp_map_fuse`` call, ``tool.viz.fuse_points``; include/sp_hip.h has the arithmetic: integer sums,
    two runs give the same bits).  Fused points come in the order of their first member row, so they stay grouped by keyframe, each
    under the keyframe that saw its voxel first.  Returns a new world dict: ``points`` (M,3), ``colours`` (M,3), ``kf_index`` and
    ``seg_ids`` (M,) -- those of the first member --, ``count`` (M,) int32 (members), ``first`` (M,) int32 (the first member's row of
    ``world``), ``label`` (Q,) int32 (per INPUT row its fused row, -1 for a row that was dropped: a non-finite coordinate, or beyond
    2^20 voxels from the origin) and ``offsets`` recomputed (host integers); every other entry (``ids``, ``align``, the ATE fields) is
    carried over.  ``render_map``, ``score_map``, ``score_map_images``, ``map_consistency`` and ``filter_map`` accept the result as it
    is (``filter_map`` compacts the four per-point tensors; ``count``, ``first`` and ``label`` then still describe the unfiltered
    fused map).  With ``world['normals']`` the result has ``normals`` (M,3): per fused point the normalised sum of its members' normals
    (``fused_normals``: integer sums, two runs give the same bits; opposite members cancel to (0, 0, 0), "no normal").  The footprint
    of a fused point is its voxel: ``radii = torch.full((M,), voxel / 2)``.  ``world`` is validated as
    ``filter_map`` does (``ValueError``).  Sizing the output takes ONE host read -- the new offsets, n_kf + 1 integers from
    ``torch.searchsorted(first, old_offsets)``, the last of which is M."""
    from ..tool import viz
    Q = _check_world(world, "fuse_map")
    if Q == 0:
        raise ValueError("fuse_map: no points")
    fused = viz.fuse_points(world['points'], world['colours'], voxel=voxel, origin=origin)
    dev = fused['first'].device
    old = torch.as_tensor(np.asarray(world['offsets'], dtype=np.int64)).to(dev)
    offsets = torch.searchsorted(fused['first'].long(), old).cpu().numpy()             # the one host read (rows beyond M hold 2^31 - 1)
    M = int(offsets[-1])
    first = fused['first'][:M]
    out = {k: v for k, v in world.items() if k not in _PER_POINT and k != 'offsets'}
    out.update(points=fused['points'][:M], colours=fused['colours'][:M], kf_index=world['kf_index'][first.long()],
               seg_ids=world['seg_ids'][first.long()], count=fused['count'][:M], first=first, label=fused['label'], offsets=offsets)
    if world.get('normals') is not None:
        out['normals'] = fused_normals(world['normals'], fused['label'], M)
    return out


def _pool(label, M, values):
    """``pool_map``'s sum: ``values`` (Q,) or (Q,k) integers added per ``label`` (Q,) into int64 (M,) or (M,k); label -1 counts nowhere."""
    lab = label.long()
    key = torch.where(lab >= 0, lab, torch.full_like(lab, M))                          # (one row beyond the map takes the dropped rows)
    out = torch.zeros((M + 1,) + tuple(values.shape[1:]), dtype=torch.int64, device=values.device).index_add_(0, key, values.long())
    return out[:M]


def fused_normals(normals, label, M):
    """The normal of every fused point: ``normals`` (Q,3) float32 of the members, ``label`` (Q,) their fused rows (-1: dropped), ``M``
    fused points.  Each component is quantised to int32 ``round(n * 2^20)`` (float64 product, ties to even; a non-finite component
    counts as 0), summed per fused point by ``pool_map``'s integer ``index_add_`` -- exact in any order, so two runs give the same bits
    --, and the sum S is normalised in float64: ``S / sqrt((S0 S0 + S1 S1) + S2 S2)``, rounded to float32 once; a zero sum stays
    (0, 0, 0).  Runs on CPU tensors too.  No host read."""
    if not torch.is_tensor(normals) or normals.dtype != torch.float32 or normals.dim() != 2 or normals.shape[1] != 3 \
            or tuple(label.shape) != (normals.shape[0],):
        raise ValueError("fused_normals: normals must be float32 (Q,3) with one label per row")
    q = torch.round(torch.nan_to_num(normals.detach().double(), nan=0.0, posinf=0.0, neginf=0.0) * _NORMAL_SCALE).to(torch.int32)
    return _unit_rows(_pool(label.to(q.device), int(M), q).double())                   # (|S| <= members * 2^20: exact in float64)


def _unit_rows(S):
    """Integer sums S (M,3) as float64, normalised: ``S / sqrt((S0 S0 + S1 S1) + S2 S2)`` rounded to float32 once; a zero sum stays 0."""
    length = torch.sqrt((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])
    unit = S / torch.where(length > 0, length, torch.ones_like(length))[:, None]
    return unit.float()


def pool_map(fused, values):
    """Per-input-row integers summed per fused point: ``fused`` is what ``fuse_map`` returned, ``values`` an integer tensor of shape
    (Q,) or (Q,k) over the rows of the map that was fused -- ``sequence_consistency(...)['counts']`` gives every fused point the agree /
    in front / behind counts of all its members.  Returns int64 (M,) or (M,k) on the values' device.  One ``index_add_`` through
    ``fused['label']``: exact, whatever the order; rows with ``label = -1`` are counted nowhere.  No host read."""
    label = fused['label']
    M = int(fused['points'].shape[0])
    if not torch.is_tensor(values) or values.is_floating_point() or values.is_complex() or values.dim() not in (1, 2) \
            or values.shape[0] != label.shape[0]:
        raise ValueError(f"pool_map: values must be integers of shape ({label.shape[0]},) or ({label.shape[0]},k), got "
                         f"{(values.dtype, tuple(values.shape)) if torch.is_tensor(values) else type(values).__name__}")
    return _pool(label, M, values)


def _threshold(radius, threshold, what):
    """(radius, threshold) as floats, the threshold defaulting to the radius; a search at ``radius`` has not seen anything farther."""
    try:
        radius = float(radius)
        threshold = radius if threshold is None else float(threshold)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: radius {radius!r}, threshold {threshold!r}: {e}") from None
    if not (radius > 0.0 and radius < float("inf")) or not threshold >= 0.0:
        raise ValueError(f"{what}: radius {radius} (finite, > 0), threshold {threshold} (>= 0)")
    if threshold > radius:
        raise ValueError(f"{what}: threshold {threshold} > radius {radius}: the search has not seen neighbours beyond its radius")
    return radius, threshold


def cloud_metrics(dist_a, dist_b, radius, threshold):
    """The 3D scores of a map against a reference cloud from two nearest-neighbour searches at ``radius``: ``dist_a`` (Qa,) the
    distance of every MAP point to its nearest reference point, ``dist_b`` (Qb,) that of every REFERENCE point to its nearest map point,
    +inf where the search found none (``nearest_points(...)['dist']``).  Returns a dict of 0-dim tensors on the distances' device.
    Exact int64 counts: ``n_a``, ``n_b`` (rows), ``found_a``, ``found_b`` (rows with a neighbour), ``within_a``, ``within_b`` (rows
    with ``dist <= threshold``).  Float64: ``accuracy`` = the mean of ``dist_a`` over its found rows and ``completion`` = the same for
    ``dist_b`` (NaN when nothing was found); ``accuracy_clipped`` / ``completion_clipped`` = the mean over ALL rows, a row without a
    neighbour counted at ``radius`` -- a hole in the map raises ``completion_clipped``, not ``completion``; ``precision`` = within_a /
    n_a; ``recall`` = within_b / n_b, the completion ratio; ``fscore`` = 2 precision recall / (precision + recall), 0 when both are 0;
    ``chamfer`` = accuracy + completion.  Sums are float64 ``torch.sum``s of the float32 distances.  ``threshold > radius`` raises
    ``ValueError``.  Pure torch: runs on CPU tensors too, and makes no host read."""
    radius, threshold = _threshold(radius, threshold, "cloud_metrics")
    out = {}
    for side, d in (('a', dist_a), ('b', dist_b)):
        if not torch.is_tensor(d) or d.dtype != torch.float32 or d.dim() != 1 or d.shape[0] == 0:
            raise ValueError(f"cloud_metrics: dist_{side} must be a non-empty float32 (Q,) tensor")
        found = d < float("inf")
        n = torch.tensor(int(d.shape[0]), dtype=torch.int64, device=d.device)
        n_found = found.sum()
        d64 = d.detach().double()
        zero = torch.zeros((), dtype=torch.float64, device=d.device)
        out['n_' + side], out['found_' + side], out['within_' + side] = n, n_found, (d <= threshold).sum()
        out['mean_' + side] = torch.where(found, d64, zero).sum() / n_found.double()
        out['clipped_' + side] = torch.where(found, d64, zero + radius).sum() / n.double()
    precision, recall = out['within_a'].double() / out['n_a'].double(), out['within_b'].double() / out['n_b'].double()
    both = precision + recall
    fscore = torch.where(both > 0, 2.0 * precision * recall / torch.where(both > 0, both, torch.ones_like(both)), torch.zeros_like(both))
    accuracy, completion = out.pop('mean_a'), out.pop('mean_b')
    out.update(accuracy=accuracy, completion=completion, accuracy_clipped=out.pop('clipped_a'), completion_clipped=out.pop('clipped_b'),
               precision=precision, recall=recall, fscore=fscore, chamfer=accuracy + completion)
    return out


def map_distance(world, reference, radius, threshold=None, origin=None):
    """The map against a reference cloud in 3D: ``world`` is any world dict ``fuse_map`` accepts (raw, filtered or fused),
    ``reference`` a dict with ``'points'`` or an (R,3) float32 tensor -- usually what ``viz.depth_image_lift`` / ``lift_depth_images``
    made of the ground-truth depths, trimmed to its valid rows.  Two ``cloud_grid`` builds and two ``nearest_points`` queries at
    ``radius`` (include/sp_hip.h has the rule): returns ``dict(to_reference, to_map, metrics)`` -- per map point its nearest reference
    point (``index``, ``dist``, ``count``), per reference point its nearest map point, and ``cloud_metrics`` of the two distances at
    ``threshold`` (default: ``radius``).  ``world`` is left untouched.  No synchronisation."""
    from ..tool import viz
    radius, threshold = _threshold(radius, threshold, "map_distance")
    _check_world(world, "map_distance")
    ref = reference.get('points') if isinstance(reference, dict) else reference
    if not torch.is_tensor(ref):
        raise ValueError("map_distance: reference must be an (R,3) float32 tensor or a dict with 'points'")
    ref_grid = viz.cloud_grid(ref, radius, origin)
    to_reference = viz.nearest_points(world['points'], ref_grid)
    map_grid = viz.cloud_grid(world['points'], radius, origin)
    to_map = viz.nearest_points(ref, map_grid)
    return dict(to_reference=to_reference, to_map=to_map, metrics=cloud_metrics(to_reference['dist'], to_map['dist'], radius, threshold))


def _mat3(x, d):
    """Rows of ``x`` (Q,3) times the rows of ``d`` (3,3), each sum as (x + y) + z: the three-term order of the kernels' contracts."""
    return torch.stack([(x[:, 0] * d[k, 0] + x[:, 1] * d[k, 1]) + x[:, 2] * d[k, 2] for k in range(3)], dim=1)


def transform_map(world, rot, trans, s=1.0):
    """``world`` moved by the similarity x -> s R x + t (``rot`` (3,3), ``trans`` (3,), ``s`` a number or 0-dim tensor -- what
    ``register_map`` / ``viz.register_clouds`` return, or any numbers): a NEW world dict whose ``points`` are computed in float64 from
    the float32 rows -- ``s ((R_k0 x + R_k1 y) + R_k2 z) + t_k``, rounded to float32 once -- and whose ``normals`` (when the world has
    them) are rotated the same way, ``(R_k0 n_x + R_k1 n_y) + R_k2 n_z``, rounded once; every other entry is carried over.  ``world`` is
    left untouched.  Pure torch: runs on CPU tensors too, and makes no host read."""
    pts = world.get('points') if isinstance(world, dict) else None
    if not torch.is_tensor(pts) or pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError("transform_map: world['points'] must be a float32 (Q,3) tensor")
    dev = pts.device
    f64 = lambda x: torch.as_tensor(x, dtype=torch.float64).detach().to(dev)          # (numbers and lists become float64 directly)
    R, t, sc = f64(rot), f64(trans).reshape(-1), f64(s)
    if tuple(R.shape) != (3, 3) or tuple(t.shape) != (3,) or sc.dim() != 0:
        raise ValueError(f"transform_map: rot {tuple(R.shape)}, trans {tuple(t.shape)}, s {tuple(sc.shape)} (want (3,3), (3,), a scalar)")
    out = dict(world)
    out['points'] = (sc * _mat3(pts.detach().double(), R) + t).float()
    nrm = world.get('normals')
    if nrm is not None:
        if not torch.is_tensor(nrm) or nrm.dtype != torch.float32 or tuple(nrm.shape) != tuple(pts.shape):
            raise ValueError(f"transform_map: world['normals'] must be a float32 tensor {tuple(pts.shape)}")
        out['normals'] = _mat3(nrm.detach().double(), R).float()
    return out


def register_map(world, reference, radius, residual=None, **kw):
    """The map moved onto a reference cloud by ICP before it is scored: ``reference`` is a dict with ``'points'`` (and maybe
    ``'normals'``) or an (R,3) float32 tensor, ``radius`` the correspondence radius.  ONE ``cloud_grid`` build over the reference and
    ONE ``viz.register_clouds`` call (``sp_cloud_register``; include/sp_hip.h has the rule) with the map's points as the queries.
    ``residual`` defaults to ``'query_plane'`` when the map has normals, else ``'plane'`` when the reference has them, else
    ``'point'``; ``**kw`` goes to ``register_clouds`` (``T0``, ``s0``, ``scale``, ``huber``, ``tol``, ``min_pairs``, ``max_iters``).
    Returns ``dict(transform=<what register_clouds returned>, world=transform_map(world, rot, trans, s))``; pass ``['world']`` to
    ``map_distance``.  ``world`` is left untouched.  No synchronisation, no host read."""
    from ..tool import viz
    _check_world(world, "register_map")
    ref = reference.get('points') if isinstance(reference, dict) else reference
    if not torch.is_tensor(ref):
        raise ValueError("register_map: reference must be an (R,3) float32 tensor or a dict with 'points'")
    ref_normals = reference.get('normals') if isinstance(reference, dict) else None
    if residual is None:
        residual = 'query_plane' if world.get('normals') is not None else ('plane' if ref_normals is not None else 'point')
    normals = {'point': None, 'plane': ref_normals, 'query_plane': world.get('normals')}.get(residual)
    if residual in ('plane', 'query_plane') and normals is None:
        raise ValueError(f"register_map: residual {residual!r} needs normals of the {'reference' if residual == 'plane' else 'map'}")
    grid = viz.cloud_grid(ref, radius)
    transform = viz.register_clouds(world['points'], grid, normals=normals, residual=residual, **kw)
    return dict(transform=transform, world=transform_map(world, transform['rot'], transform['trans'], transform['s']))


def map_neighbours(world, radius, origin=None):
    """Every map point against the other points of the map: ``index`` (Q,) int32 the nearest OTHER point within ``radius`` (-1: none),
    ``dist`` (Q,) float32 its distance -- the map's spacing -- and ``count`` (Q,) int32 the other points within ``radius``: Open3D's
    ``remove_radius_outlier(nb_points, radius)`` keeps the rows with ``count >= nb_points``.  One ``cloud_grid`` build and one
    ``nearest_points`` query with ``skip_self``.  No synchronisation."""
    from ..tool import viz
    _check_world(world, "map_neighbours")
    grid = viz.cloud_grid(world['points'], radius, origin)
    return viz.nearest_points(grid['points'], grid, skip_self=True)


def estimate_normals(cloud, radius, k=16, view_centres=None, owner=None):
    """Normals for a cloud that has none: ``cloud`` is a world dict, a ``dict(points=...)`` or an (R,3) float32 tensor -- lifted ground
    truth, a fused map whose members carried no normals, a scan, the map of another sequence.  ``viz.cloud_normals``: ONE grid build at
    ``radius``, ONE ``sp_cloud_grid_knn`` and ONE ``sp_cloud_normals`` launch (include/sp_hip.h has the rule): per point the direction
    of least spread of its up to ``k`` (1 .. 32) nearest points within ``radius``, itself included.  ``view_centres`` (3,) or (V,3)
    float32 and ``owner`` (R,) int32 turn the normal of row i towards ``view_centres[owner[i]]``; without them the component of
    largest magnitude is positive.  Returns a NEW dict: the cloud's entries and ``'normals'`` (R,3) float32 (NaN where fewer than
    three points were in reach, or they are coincident or collinear: ``sp_cloud_register`` ignores such rows), ``'curvature'`` (R,)
    float32 (l0 / (l0 + l1 + l2), the surface variation) and ``'normals_used'`` (R,) int32.  ``register_map`` takes the result as its
    reference as it is and then picks the ``'plane'`` residual; ``write_ply`` and ``transform_map`` take it too.  The lifted ground
    truth of a sequence, every point turned towards the camera that saw it, with no host read::

        lifted = viz.lift_depth_images(gt_depths, Ks, gt_poses)                # points (R,3) at capacity, offsets (V+1,) on the device
        row = torch.arange(R, device=dev)
        owner = torch.bucketize(row, lifted['offsets'][1:], right=True).int()  # (V for the spare rows: no viewpoint)
        points = torch.where((row < lifted['offsets'][-1])[:, None], lifted['points'], nan)    # the spare rows are uninitialised: NaN is never found
        reference = estimate_normals(points, radius, view_centres=gt_poses[:, :3, 3].contiguous(), owner=owner)
        moved = register_map(world, reference, radius)                         # residual 'plane'

    No synchronisation."""
    from ..tool import viz
    pts = cloud.get('points') if isinstance(cloud, dict) else cloud
    if not torch.is_tensor(pts):
        raise ValueError("estimate_normals: cloud must be an (R,3) float32 tensor or a dict with 'points'")
    try:
        radius = float(radius)
    except (TypeError, ValueError) as e:
        raise ValueError(f"estimate_normals: radius {radius!r}: {e}") from None
    found = viz.cloud_normals(pts, radius, k=k, toward=view_centres, owner=owner)
    out = dict(cloud) if isinstance(cloud, dict) else dict(points=pts)
    out.update(normals=found['normals'], curvature=found['curvature'], normals_used=found['used'])
    return out


def statistical_outliers(world, radius, k=16, std_ratio=2.0, knn=None):
    """The project's statistical outlier rule (the idea of the well-known point-cloud filter of that name; no equality with any other
    library's result is claimed): every map point's mean distance to its up to ``k`` (1 .. 32) nearest OTHER points within ``radius``
    against the cloud's own mean and deviation of that figure.  One ``cloud_grid`` build and one ``viz.nearest_k`` with ``skip_self``
    (or ``knn``: what such a call returned for this map, reused).
        mean_dist[i] = the float64 mean of the finite entries of ``knn['dist'][i]``;  +inf where there is none (no point within radius)
        mu, sigma    = the mean and the population deviation (divisor n) of ``mean_dist`` over its finite rows
        threshold    = mu + std_ratio * sigma;   keep[i] = mean_dist[i] <= threshold     (a row with no neighbour is never kept)
    Returns ``dict(mean_dist (Q,) float64, keep (Q,) bool, mu, sigma, threshold (0-dim float64), knn)``; pass ``keep`` to
    ``select_map``.  The arithmetic is plain torch: with ``knn`` given it runs on CPU tensors too.  No synchronisation, no host read."""
    from ..tool import viz
    Q = _check_world(world, "statistical_outliers")
    try:
        std_ratio = float(std_ratio)
    except (TypeError, ValueError) as e:
        raise ValueError(f"statistical_outliers: std_ratio {std_ratio!r}: {e}") from None
    if not (0.0 <= std_ratio < float("inf")):
        raise ValueError(f"statistical_outliers: std_ratio {std_ratio} (finite, >= 0)")
    if knn is None:
        viz._list_length(k, "statistical_outliers")                                    # (before the build)
        grid = viz.cloud_grid(world['points'], radius)
        knn = viz.nearest_k(grid['points'], grid, k, skip_self=True)
    dist = knn.get('dist') if isinstance(knn, dict) else None
    if not torch.is_tensor(dist) or dist.dtype != torch.float32 or dist.dim() != 2 or dist.shape[0] != Q or dist.shape[1] < 1:
        raise ValueError(f"statistical_outliers: knn['dist'] must be float32 ({Q},k)")
    d = dist.detach().double()
    finite = d < float("inf")
    n = finite.sum(dim=1)
    total = torch.where(finite, d, torch.zeros_like(d)).sum(dim=1)
    has = n > 0
    inf = torch.full_like(total, float("inf"))
    mean_dist = torch.where(has, total / torch.where(has, n, torch.ones_like(n)).double(), inf)
    rows = has.sum().double()
    zero = torch.zeros_like(total)
    mu = torch.where(has, mean_dist, zero).sum() / rows
    dev2 = torch.where(has, mean_dist - mu, zero)
    sigma = torch.sqrt((dev2 * dev2).sum() / rows)
    threshold = mu + std_ratio * sigma
    return dict(mean_dist=mean_dist, keep=mean_dist <= threshold, mu=mu, sigma=sigma, threshold=threshold, knn=knn)


def _three(x, what):
    """Three finite numbers as Python floats (a list, an array or a tensor: a device tensor costs one host read)."""
    try:
        v = [float(a) for a in torch.as_tensor(x, dtype=torch.float64).detach().reshape(-1).tolist()]
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{what} {x!r}: {e}") from None
    if len(v) != 3 or not all(abs(a) < float("inf") for a in v):
        raise ValueError(f"{what} {x!r} (three finite numbers)")
    return v


def _voxel_trunc(voxel, trunc, what):
    """``voxel`` and ``trunc`` (default 4 voxels) as finite floats > 0."""
    try:
        voxel = float(voxel)
        trunc = 4.0 * voxel if trunc is None else float(trunc)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: voxel {voxel!r}, trunc {trunc!r}: {e}") from None
    if not (0.0 < voxel < float("inf")) or not (0.0 < trunc < float("inf")):
        raise ValueError(f"{what}: voxel {voxel}, trunc {trunc} (finite, > 0)")
    return voxel, trunc


def tsdf_volume(lo, hi, voxel, trunc=None, colour=True, device="cuda"):
    """An empty signed-distance volume over the box ``lo`` .. ``hi`` (three numbers each): ``ceil((hi - lo) / voxel)`` nodes per axis, at
    least one, node (ix,iy,iz) at ``lo + (i + 0.5) voxel``.  ``trunc``: the truncation distance (default ``4 * voxel``).  Returns
    ``dict(tsdf, weight (nz,ny,nx) float32 zeros, colour (nz,ny,nx,3) float32 zeros or None, origin (three floats), voxel, trunc, dims
    (nx, ny, nz))`` -- what ``fuse_tsdf`` / ``viz.tsdf_integrate`` update in place and ``extract_mesh`` cuts.  Raises ``ValueError`` for a
    box of more than 2^30 nodes, before anything is allocated."""
    voxel, trunc = _voxel_trunc(voxel, trunc, "tsdf_volume")
    lo, hi = _three(lo, "tsdf_volume: lo"), _three(hi, "tsdf_volume: hi")
    if any(h < l for l, h in zip(lo, hi)):
        raise ValueError(f"tsdf_volume: box {lo} .. {hi}")
    dims = tuple(max(1, int(np.ceil((h - l) / voxel))) for l, h in zip(lo, hi))
    if dims[0] * dims[1] * dims[2] > _lib.SP_TSDF_MAX_NODES:
        raise ValueError(f"tsdf_volume: {dims[0]}x{dims[1]}x{dims[2]} nodes are beyond the kernels' limit of 2^30; use a larger voxel or a smaller box")
    nx, ny, nz = dims
    return dict(tsdf=torch.zeros(nz, ny, nx, dtype=torch.float32, device=device), weight=torch.zeros(nz, ny, nx, dtype=torch.float32, device=device),
                colour=torch.zeros(nz, ny, nx, 3, dtype=torch.float32, device=device) if colour else None, origin=tuple(lo), voxel=voxel, trunc=trunc,
                dims=dims)


def _finite_extent(points, valid=None):
    """(lo, hi) of the rows of ``points`` (Q,3) whose coordinates are all finite (and ``valid``): two device reductions, ONE host read."""
    ok = torch.isfinite(points).all(dim=1)
    if valid is not None:
        ok = ok & valid
    inf = torch.full_like(points, float("inf"))
    lo = torch.where(ok[:, None], points, inf).amin(dim=0)
    hi = torch.where(ok[:, None], points, -inf).amax(dim=0)
    both = torch.stack((lo, hi)).double().tolist()                                     # the one host read
    if not all(abs(a) < float("inf") for row in both for a in row):
        raise ValueError("no finite point to take the bounds from")
    return both[0], both[1]


def fuse_tsdf(depths, Ks, poses, voxel, bounds=None, images=None, volume=None, trunc=None, z_min=None, depth_max=float("inf")):
    """Depth images fused into a signed-distance volume (``viz.tsdf_integrate``: ONE ``sp_tsdf_integrate`` launch; include/sp_hip.h has
    the rule): ``depths`` (V,H,W) float32 -- the keyframes' own (``sequence_tsdf``) or ground truth, for a ground-truth surface --, ``Ks``
    (V,3,3) or (3,3), ``poses`` (V,4,4) camera-to-world, ``images`` (V,3,H,W) float32 or None.  ``volume``: an existing volume to continue
    (``voxel``, ``bounds`` and ``trunc`` are then ignored); else a new one over ``bounds`` = (lo, hi), or -- ``bounds=None`` -- over the
    finite extent of the lifted depths (``viz.lift_depth_images``; one host read) padded by ``trunc`` (default ``4 * voxel``), with a
    colour iff there are images.  Returns the volume."""
    from ..tool import viz
    Ks, poses = _view_cameras(Ks, poses, "fuse_tsdf")
    z_min = viz.Z_MIN if z_min is None else z_min
    try:
        depth_max = float(depth_max)
    except (TypeError, ValueError) as e:
        raise ValueError(f"fuse_tsdf: depth_max {depth_max!r}: {e}") from None
    if not depth_max > 0.0:
        raise ValueError(f"fuse_tsdf: depth_max {depth_max} (> 0; inf allowed)")
    if volume is None:
        voxel, trunc = _voxel_trunc(voxel, trunc, "fuse_tsdf")
        if not torch.is_tensor(depths) or depths.dim() != 3 or depths.dtype != torch.float32 or depths.shape[0] != poses.shape[0]:
            raise ValueError(f"fuse_tsdf: depths must be float32 (V,H,W) for {poses.shape[0]} views, got "
                             f"{tuple(depths.shape) if torch.is_tensor(depths) else type(depths).__name__}")
        if bounds is None:
            cap = min(depth_max, 3.0e38)
            lifted = viz.lift_depth_images(depths, Ks, poses.float(), depth_trunc=cap)
            rows = torch.arange(lifted['points'].shape[0], device=lifted['points'].device)
            try:
                lo, hi = _finite_extent(lifted['points'], rows < lifted['offsets'][-1])
            except ValueError as e:
                raise ValueError(f"fuse_tsdf: {e}") from None
            lo, hi = [a - trunc for a in lo], [a + trunc for a in hi]
        else:
            try:
                lo, hi = bounds
            except (TypeError, ValueError):
                raise ValueError(f"fuse_tsdf: bounds {bounds!r} (a pair (lo, hi))") from None
        volume = tsdf_volume(lo, hi, voxel, trunc, colour=images is not None, device=depths.device)
    return viz.tsdf_integrate(volume, depths, Ks, poses, images=images, z_min=z_min, depth_max=depth_max)


def sequence_tsdf(world, result, voxel, trunc=None, depth_max=float("inf")):
    """The surface a sequence saw: the keyframes' own depth images (``sequence_consistency``'s: ``viz.keyframe_depths`` on the archive,
    times the alignment scale when ``world`` carries ``align``), their Ks and their poses in the map's frame, fused into ONE volume over
    the finite extent of ``world['points']`` padded by ``trunc`` (default ``4 * voxel``; one host read), coloured from the keyframes'
    images.  ``world`` is ``sequence_map`` of ``result`` (``run_sequence(..., keep_keyframes=True)``).  Returns the volume plus ``depths``
    (n,H,W): pass it to ``extract_mesh``."""
    voxel, trunc = _voxel_trunc(voxel, trunc, "sequence_tsdf")
    views = _sequence_views(world, result, "sequence_tsdf")
    archive = result['kf_archive']
    images = torch.stack([archive[i]['kf'].image[:3].detach().float() for i in world['ids']]).contiguous()
    try:
        lo, hi = _finite_extent(world['points'])
    except ValueError as e:
        raise ValueError(f"sequence_tsdf: {e}") from None
    volume = fuse_tsdf(views['depths'], views['Ks'], views['poses'], voxel, bounds=([a - trunc for a in lo], [a + trunc for a in hi]), images=images,
                       trunc=trunc, depth_max=depth_max)
    volume['depths'] = views['depths']
    return volume


def extract_mesh(volume, min_weight=1.0):
    """The zero level set of a volume as a triangle mesh (``viz.tsdf_mesh``: ``sp_tsdf_mesh``, marching tetrahedra; one host read of the
    two counts).  Returns ``dict(points (M,3), colours (M,3) float32 -- zeros for a volume without colour --, faces (F,3) int32 into
    ``points``, looking into free space, and kf_index, seg_ids (M,) int32 = -1, offsets = [0, M])``: the vertices are a cloud, so
    ``map_distance``, ``register_map``, ``estimate_normals``, ``render_map`` and ``write_ply`` accept the dict as it is."""
    from ..tool import viz
    found = viz.tsdf_mesh(volume, min_weight=min_weight)
    points = found['vertices']
    M, dev = int(points.shape[0]), points.device
    colours = found['colours'] if found['colours'] is not None else torch.zeros(M, 3, dtype=torch.float32, device=dev)
    none = torch.full((M,), -1, dtype=torch.int32, device=dev)
    return dict(points=points, colours=colours, faces=found['faces'], kf_index=none, seg_ids=none.clone(), offsets=np.array([0, M], dtype=np.int64))


def _mesh_parts(mesh, what):
    """(points (M,3) float32, faces (F,3) int32) of a mesh dict -- ``extract_mesh``'s, ``read_ply``'s or ``clean_mesh``'s."""
    pts = mesh.get('points') if isinstance(mesh, dict) else None
    faces = mesh.get('faces') if isinstance(mesh, dict) else None
    if not torch.is_tensor(pts) or pts.dtype != torch.float32 or pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"{what}: mesh['points'] must be a float32 (M,3) tensor")
    if not torch.is_tensor(faces) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: mesh['faces'] must be an int32 (F,3) tensor")
    if faces.device != pts.device:
        raise ValueError(f"{what}: points on {pts.device}, faces on {faces.device}")
    if pts.shape[0] < 1 or faces.shape[0] < 1:
        raise ValueError(f"{what}: a mesh of {int(pts.shape[0])} vertices and {int(faces.shape[0])} faces")
    return pts, faces


def _face_records(mesh, records, what, cross=False):
    """``records`` checked against the mesh, or ``mesh_faces(mesh)``."""
    pts, faces = _mesh_parts(mesh, what)
    if records is None:
        return mesh_faces(mesh, cross=cross)
    F = int(faces.shape[0])
    need = ('area', 'normals', 'state', 'area_max') + (('cross',) if cross else ())
    if not isinstance(records, dict) or any(not torch.is_tensor(records.get(k)) for k in need):
        raise ValueError(f"{what}: records must be what mesh_faces{'(mesh, cross=True)' if cross else ''} returned (tensors {need})")
    if tuple(records['state'].shape) != (F,) or records['state'].dtype != torch.uint8 or tuple(records['area'].shape) != (F,) \
            or (cross and (tuple(records['cross'].shape) != (F, 3) or records['cross'].dtype != torch.float64)):
        raise ValueError(f"{what}: records of another mesh ({F} faces here)")
    return records


def mesh_faces(mesh, cross=False):
    """One record per face of a mesh dict (``points`` (M,3) float32, ``faces`` (F,3) int32): ONE ``sp_mesh_faces`` launch
    (``tool.viz.mesh_faces``; include/sp_hip.h has the rule).  Returns ``dict(area (F,) float64, normals (F,3) float32, state (F,) uint8 --
    0 valid, 1 an index outside the vertices, 2 a repeated index, 3 a non-finite coordinate, 4 zero area --, counts (5,) int64 (faces per
    state), area_max, area_total (0-dim float64))`` and, with ``cross``, the raw cross products (F,3) float64.  ``area_total`` is the
    ``torch.sum`` of ``area``: the one figure here whose last bits depend on the order of a sum.  No synchronisation."""
    from ..tool import viz
    pts, faces = _mesh_parts(mesh, "mesh_faces")
    found = viz.mesh_faces(pts, faces, cross=cross)
    summary = found.pop('summary')
    found.update(counts=summary[:5], area_max=summary[5:].view(torch.float64)[0], area_total=torch.sum(found['area']))
    return found


def _select_faces(mesh, pts, faces, keep, what):
    """The selection ``clean_mesh`` and ``cull_mesh`` share: the faces where ``keep`` (F,) bool holds -- each with its three indices inside
    the vertices --, then the vertices they reference, both in their order, re-indexed; ``colours`` and ``normals`` carried along."""
    M = int(pts.shape[0])
    kept_faces = torch.nonzero(keep).reshape(-1)
    kept = faces[kept_faces].long()
    used = torch.zeros(M, dtype=torch.bool, device=pts.device)
    used[kept.reshape(-1)] = True
    new_index = torch.cumsum(used.long(), dim=0) - 1
    kept_vertices = torch.nonzero(used).reshape(-1)
    Mk = int(kept_vertices.shape[0])
    out = dict(points=pts[kept_vertices], faces=new_index[kept].to(torch.int32), kept_vertices=kept_vertices, kept_faces=kept_faces)
    for key in ('colours', 'normals'):
        if mesh.get(key) is not None:
            if not torch.is_tensor(mesh[key]) or tuple(mesh[key].shape) != (M, 3):
                raise ValueError(f"{what}: mesh['{key}'] must be a tensor ({M},3)")
            out[key] = mesh[key][kept_vertices]
    none = torch.full((Mk,), -1, dtype=torch.int32, device=pts.device)
    out.update(kf_index=none, seg_ids=none.clone(), offsets=np.array([0, Mk], dtype=np.int64))
    return out


def clean_mesh(mesh, records=None):
    """``mesh`` without its degenerate triangles: the faces whose state is not 0 dropped (``mesh_faces``; ``records``: what it returned
    for this mesh, reused), then the vertices no kept face references; the order of both is preserved and duplicate positions are not
    welded.  Plain torch over ``state`` (boolean selection and a cumulative sum for the new indices): with ``records`` it runs on CPU
    tensors too.  Returns a NEW dict: ``points``, ``colours``, ``normals`` (when present), ``faces`` (re-indexed, int32), ``kept_vertices``
    and ``kept_faces`` (int64: the surviving rows of the input), and ``kf_index`` / ``seg_ids`` = -1, ``offsets`` = [0, M'] as
    ``extract_mesh`` forms them.  Two host reads on the device: the sizes of the two boolean selections."""
    pts, faces = _mesh_parts(mesh, "clean_mesh")
    state = _face_records(mesh, records, "clean_mesh")['state'].to(pts.device)
    return _select_faces(mesh, pts, faces, state == 0, "clean_mesh")                   # (state 0: every index is inside the vertices)


_CROSS_SCALE = 2.0 ** 30           # mesh_normals: face cross products are summed as int64 round(c * (2^30 / c_max))


def mesh_normals(mesh, records=None):
    """Area-weighted vertex normals, bitwise repeatable: a NEW dict, ``mesh`` plus ``'normals'`` (M,3) float32.  Per valid face its cross
    product c (``mesh_faces(mesh, cross=True)``, or ``records``: what that returned, reused -- then CPU tensors work too), whose length is
    twice the face's area, is quantised per component to int64 ``q = round(c * (2^30 / c_max))`` (float64, ties to even; ``c_max = 2
    area_max``, so |q| <= 2^30), summed per vertex over the face's three corners by ``pool_map``'s integer ``index_add_`` -- exact in
    any order --, and the sum is normalised in float64 exactly as ``fused_normals`` does; a vertex of no valid face keeps (0, 0, 0).
    Faces look into free space (``extract_mesh``), so do the normals.  No host read."""
    pts, faces = _mesh_parts(mesh, "mesh_normals")
    rec = _face_records(mesh, records, "mesh_normals", cross=True)
    dev = pts.device
    c_max = 2.0 * rec['area_max'].to(dev).double()
    scale = torch.where(c_max > 0, _CROSS_SCALE / torch.where(c_max > 0, c_max, torch.ones_like(c_max)), torch.zeros_like(c_max))
    q = torch.round(rec['cross'].to(dev) * scale).to(torch.int64)
    valid = (rec['state'].to(dev) == 0)[:, None]
    label = torch.where(valid, faces.long(), torch.full_like(faces, -1, dtype=torch.int64)).t().reshape(-1)     # corner 0 of every face, then 1, then 2
    out = dict(mesh)
    out['normals'] = _unit_rows(_pool(label, int(pts.shape[0]), q.repeat(3, 1)).double())
    return out


def _n_or_density(n, density, what):
    if (n is None) == (density is None):
        raise ValueError(f"{what}: exactly one of n and density must be given")
    try:
        if n is not None:
            if int(n) != n or int(n) < 1:
                raise ValueError("n must be a whole number >= 1")
            return int(n), None
        density = float(density)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: n {n!r}, density {density!r}: {e}") from None
    if not (0.0 < density < float("inf")):
        raise ValueError(f"{what}: density {density} (finite, > 0)")
    return None, density


def _density_of(n, records, what):
    """``n`` samples over the records' total area: one host read."""
    total = float(records['area_total'])
    if not (0.0 < total < float("inf")):
        raise ValueError(f"{what}: a mesh of total area {total} cannot take n = {n} samples")
    return n / total


def sample_mesh(mesh, n=None, density=None, seed=0, records=None):
    """The mesh as an area-uniform cloud with exact normals: ``mesh_faces`` then ``tool.viz.mesh_sample`` (``sp_mesh_sample``;
    include/sp_hip.h has the rule): every valid face i takes ``floor(area_i density + U_i)`` samples -- stochastic rounding by the
    face's own seeded hash, so a long flat triangle takes its share and a small one its chance --, each a seeded uniform point of the
    triangle, with the face's unit normal and the interpolated vertex colour.  Exactly one of ``density`` (samples per unit area) and
    ``n`` must be given; ``n`` means ``density = n / area_total``, which costs ONE MORE host read, and the row count is then ``n`` give or
    take the stochastic rounding (a standard deviation of at most sqrt(F) / 2), not ``n`` exactly.  The same mesh, density and ``seed`` (any 64
    bits) give the same bits.  ``records``: what ``mesh_faces`` returned for this mesh, reused.  Returns a world dict -- ``points``,
    ``colours`` (zeros without vertex colours), ``normals`` (N,3) float32, ``face`` (N,) int32 (the row of ``mesh['faces']``),
    ``kf_index`` / ``seg_ids`` (N,) int32 = -1, ``offsets`` = [0, N] -- that ``map_distance``, ``register_map`` (which then picks the
    ``'plane'`` residual for a reference), ``render_map`` and ``write_ply`` accept as it is.  One host read of the row count."""
    from ..tool import viz
    n, density = _n_or_density(n, density, "sample_mesh")
    viz._density_seed(1.0 if density is None else density, seed, "sample_mesh")
    pts, faces = _mesh_parts(mesh, "sample_mesh")
    colours = mesh.get('colours')
    if colours is not None and (not torch.is_tensor(colours) or colours.dtype != torch.float32 or tuple(colours.shape) != tuple(pts.shape)):
        raise ValueError(f"sample_mesh: mesh['colours'] must be a float32 tensor {tuple(pts.shape)}")
    rec = _face_records(mesh, records, "sample_mesh")
    if n is not None:
        density = _density_of(n, rec, "sample_mesh")
    found = viz.mesh_sample(pts, faces, rec, density, seed=seed, colours=colours)
    N, dev = int(found['points'].shape[0]), pts.device
    none = torch.full((N,), -1, dtype=torch.int32, device=dev)
    return dict(points=found['points'], colours=found['colours'] if colours is not None else torch.zeros(N, 3, dtype=torch.float32, device=dev),
                normals=found['normals'], face=found['face'], kf_index=none, seg_ids=none.clone(), offsets=np.array([0, N], dtype=np.int64))


def mesh_distance(mesh, reference_mesh, radius, threshold=None, n=None, density=None, seed=0):
    """Surface against surface: both meshes sampled at ONE density per area (``sample_mesh``), then ``map_distance`` on the two clouds --
    accuracy, completion, completion ratio (``recall``) and the rest of ``cloud_metrics`` at ``threshold`` (default ``radius``).  Exactly
    one of ``density`` and ``n``; with ``n`` the density comes from the REFERENCE's area (``n / area_total``, one host read) and both
    meshes are sampled at it.  ``seed``: one integer for both samplings, or a pair (mesh, reference).  Returns ``map_distance``'s dict
    plus ``samples`` and ``reference_samples`` (the two world dicts) and ``density``."""
    radius, threshold = _threshold(radius, threshold, "mesh_distance")
    n, density = _n_or_density(n, density, "mesh_distance")
    seeds = tuple(seed) if isinstance(seed, (tuple, list)) else (seed, seed)
    if len(seeds) != 2:
        raise ValueError(f"mesh_distance: seed {seed!r} (an integer, or a pair)")
    _mesh_parts(mesh, "mesh_distance")
    ref_records = _face_records(reference_mesh, None, "mesh_distance")
    if n is not None:
        density = _density_of(n, ref_records, "mesh_distance")
    samples = sample_mesh(mesh, density=density, seed=seeds[0])
    reference_samples = sample_mesh(reference_mesh, density=density, seed=seeds[1], records=ref_records)
    out = map_distance(samples, reference_samples, radius, threshold=threshold)
    out.update(samples=samples, reference_samples=reference_samples, density=density)
    return out


def render_surface(volume, Ks, poses, size, z_max, min_weight=1.0, step=None):
    """The fused surface seen from V cameras: ``render_map``'s counterpart for a volume (``fuse_tsdf`` / ``sequence_tsdf``), ONE
    ``sp_tsdf_raycast`` launch (``tool.viz.tsdf_raycast``; include/sp_hip.h has the rule).  ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4)
    camera-to-world in the volume's frame, ``size`` = (H, W); every ray is sampled every ``step`` (default: one voxel) of camera depth up
    to ``z_max``.  Returns dict(depth (V,H,W) float32 -- the zero crossing, 0 without a hit --, normals (V,H,W,3) float32 in the volume's
    frame, facing the cameras that saw the surface, NaN without a hit or next to unobserved cells, image (V,H,W,3) uint8 -- zeros for a
    volume without colour --, index (V,H,W) int32 -- the lower node of the cell behind the surface, -1 without a hit).  No synchronisation."""
    from ..tool import viz
    Ks, poses = _view_cameras(Ks, poses, "render_surface")
    H, W = size
    out = viz.tsdf_raycast(volume, Ks, poses, H, W, z_max, min_weight=min_weight, step=step)
    if 'image' not in out:
        out['image'] = torch.zeros(*out['index'].shape, 3, dtype=torch.uint8, device=out['index'].device)
    return out


def _surface_step(volume, step, what):
    """``step`` (default: the volume's voxel) as a finite float > 0."""
    try:
        step = float(volume['voxel'] if step is None else step)
    except (TypeError, ValueError, KeyError) as e:
        raise ValueError(f"{what}: step {step!r} for volume {type(volume).__name__}: {e}") from None
    if not (0.0 < step < float("inf")):
        raise ValueError(f"{what}: step {step} (finite, > 0)")
    return step


def score_surface(volume, gt_depths, Ks, gt_poses, min_depth=0.2, max_depth=5.0, min_weight=1.0, step=None):
    """The fused surface against ground-truth depth images: ``score_map`` for a volume.  The surface is ray-cast into each of the V
    ground-truth views up to ``z_max = max_depth + step`` (``render_surface``'s launch, depth and index only) and scored where a ray hit
    (``index >= 0``) and ``min_depth <= gt <= max_depth``.  Returns ``score_map``'s dict (metrics (V,12), columns, coverage).  No
    synchronisation."""
    from ..tool import viz
    Ks, gt_poses = _view_cameras(Ks, gt_poses, "score_surface")
    V, H, W = _target_depths(gt_depths, gt_poses, min_depth, max_depth, "score_surface")
    step = _surface_step(volume, step, "score_surface")
    viz._on_device(gt_depths)
    out = viz.tsdf_raycast(volume, Ks, gt_poses, H, W, float(max_depth) + step, min_weight=min_weight, step=step, normals=False, image=False)
    return _depth_scores(out['depth'], out['index'] >= 0, gt_depths, min_depth, max_depth)


def score_surface_images(volume, images, Ks, poses, z_max, min_weight=1.0, step=None):
    """The fused surface's colour views against real images: ``score_map_images`` for a volume with colour.  ``images`` (V,3,H,W) float32
    in 0..1; one ``sp_tsdf_raycast`` launch (image and index) plus ONE ``sp_image_metrics`` launch over the pixels a ray hit.  Returns
    ``score_map_images``' dict (sums, psnr, l1, coverage).  No synchronisation."""
    from ..tool import viz
    Ks, poses = _view_cameras(Ks, poses, "score_surface_images")
    H, W = _target_images(images, poses, "score_surface_images")
    viz._on_device(images)
    out = viz.tsdf_raycast(volume, Ks, poses, H, W, z_max, min_weight=min_weight, step=step, depth=False, normals=False, image=True)
    return _image_scores(out['image'], images, out['index'])


def _mesh_colours(mesh, pts, what):
    """``mesh['colours']`` as the float32 (M,3) vertex colours of the mesh, or None."""
    colours = mesh.get('colours')
    if colours is not None and (not torch.is_tensor(colours) or colours.dtype != torch.float32 or tuple(colours.shape) != tuple(pts.shape)):
        raise ValueError(f"{what}: mesh['colours'] must be a float32 tensor {tuple(pts.shape)}")
    return colours


def render_mesh(mesh, Ks, poses, size, cull=False, records=None):
    """The mesh seen from V cameras: ``render_surface``'s counterpart for a triangle mesh -- ``extract_mesh``'s, ``clean_mesh``'s, one moved
    by ``transform_map``, or a ground-truth model from ``read_ply`` --, ONE ``sp_mesh_render`` call (``tool.viz.mesh_render``;
    include/sp_hip.h has the rule).  ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4) camera-to-world in the mesh's frame, ``size`` = (H, W);
    ``cull=True`` keeps only faces seen from their front.  The face normals come from ``mesh_faces`` (one more launch) unless
    ``records``, what it returned for this mesh, is passed.  Returns ``render_surface``'s dict: depth (V,H,W) float32 -- 0 where no face
    lies --, normals (V,H,W,3) float32, the winning face's unit normal in the mesh's frame (NaN there; zeros for a degenerate winner),
    image (V,H,W,3) uint8 -- vertex colours interpolated perspective-correctly, zeros for a mesh without colours --, index (V,H,W) int32 --
    the winning row of ``mesh['faces']``, -1 there.  ``render_mesh(gt_mesh, Ks, gt_poses, (H, W))['depth']`` is the ground-truth depth
    ``score_map``, ``score_surface``, ``map_consistency`` and ``fuse_tsdf`` take.  No synchronisation."""
    from ..tool import viz
    Ks, poses = _view_cameras(Ks, poses, "render_mesh")
    pts, faces = _mesh_parts(mesh, "render_mesh")
    colours = _mesh_colours(mesh, pts, "render_mesh")
    H, W = size
    viz._on_device(pts, faces)
    rec = _face_records(mesh, records, "render_mesh")
    out = viz.mesh_render(pts, faces, Ks, poses, H, W, colours=colours, face_normals=rec['normals'], cull=bool(cull))
    if 'image' not in out:
        out['image'] = torch.zeros(*out['index'].shape, 3, dtype=torch.uint8, device=out['index'].device)
    return out


def score_mesh(mesh, gt_depths, Ks, gt_poses, min_depth=0.2, max_depth=5.0, cull=False):
    """The mesh against ground-truth depth images: ``score_surface`` for a triangle mesh.  The mesh is rasterised into each of the V
    ground-truth views (``render_mesh``'s call, depth and index only) and scored where a face won the pixel (``index >= 0``) and
    ``min_depth <= gt <= max_depth``.  Returns ``score_map``'s dict (metrics (V,12), columns, coverage).  No synchronisation."""
    from ..tool import viz
    Ks, gt_poses = _view_cameras(Ks, gt_poses, "score_mesh")
    V, H, W = _target_depths(gt_depths, gt_poses, min_depth, max_depth, "score_mesh")
    pts, faces = _mesh_parts(mesh, "score_mesh")
    viz._on_device(gt_depths, pts, faces)
    out = viz.mesh_render(pts, faces, Ks, gt_poses, H, W, cull=bool(cull))
    return _depth_scores(out['depth'], out['index'] >= 0, gt_depths, min_depth, max_depth)


def score_mesh_images(mesh, images, Ks, poses, cull=False):
    """The mesh's colour views against real images: ``score_surface_images`` for a mesh with vertex colours.  ``images`` (V,3,H,W) float32
    in 0..1; one ``sp_mesh_render`` call (image and index) plus ONE ``sp_image_metrics`` launch over the pixels a face won.  Returns
    ``score_map_images``' dict (sums, psnr, l1, coverage).  No synchronisation."""
    from ..tool import viz
    Ks, poses = _view_cameras(Ks, poses, "score_mesh_images")
    H, W = _target_images(images, poses, "score_mesh_images")
    pts, faces = _mesh_parts(mesh, "score_mesh_images")
    colours = _mesh_colours(mesh, pts, "score_mesh_images")
    if colours is None:
        raise ValueError("score_mesh_images: the mesh has no colours")
    viz._on_device(images, pts, faces)
    out = viz.mesh_render(pts, faces, Ks, poses, H, W, colours=colours, cull=bool(cull), depth=False, image=True)
    return _image_scores(out['image'], images, out['index'])


def visible_faces(mesh, Ks, poses, size, cull=False, index=None):
    """Which faces of the mesh the cameras see: ``dict(pixels (F,) int64, views (F,) int32)`` -- the pixels each face wins over all V views
    and the number of views in which it wins at least one --, both integer ``bincount``s of ``render_mesh``'s ``index``: exact in any
    order.  ``index``: a (V,H,W) int32 face image of this mesh made before (``render_mesh``'s, or any rasteriser's), reused -- then no
    view is rendered, ``Ks``, ``poses``, ``size`` and ``cull`` are not read, and CPU tensors work too.  No synchronisation."""
    pts, faces = _mesh_parts(mesh, "visible_faces")
    F = int(faces.shape[0])
    if index is None:
        from ..tool import viz
        Ks, poses = _view_cameras(Ks, poses, "visible_faces")
        H, W = size
        index = viz.mesh_render(pts, faces, Ks, poses, H, W, cull=bool(cull), depth=False)['index']
    elif not torch.is_tensor(index) or index.dtype != torch.int32 or index.dim() != 3:
        raise ValueError("visible_faces: index must be an int32 (V,H,W) tensor")
    V = int(index.shape[0])
    # row v of the table counts into its own F + 1 bins (bin 0: the pixels no face won)
    flat = (index.long() + 1 + (F + 1) * torch.arange(V, device=index.device)[:, None, None]).reshape(-1)
    per_view = torch.bincount(flat, minlength=V * (F + 1)).reshape(V, F + 1)[:, 1:]
    return dict(pixels=per_view.sum(dim=0), views=(per_view > 0).sum(dim=0).to(torch.int32))


def cull_mesh(mesh, Ks, poses, size, min_pixels=1, cull=False, visible=None):
    """The mesh reduced to what the cameras saw, as benchmarks cull a ground-truth model before surface-against-surface scores: the faces
    with ``visible_faces(...)['pixels'] >= min_pixels`` (a whole number >= 1), then the vertices they reference -- ``clean_mesh``'s
    selection: order kept, re-indexed, ``colours`` and ``normals`` carried along, ``kept_faces`` and ``kept_vertices`` (int64: the
    surviving rows of the input) reported.  ``visible``: what ``visible_faces`` returned for this mesh, reused -- then plain torch, and
    CPU tensors work too.  Two host reads: the sizes of the two boolean selections."""
    pts, faces = _mesh_parts(mesh, "cull_mesh")
    try:
        if int(min_pixels) != min_pixels or int(min_pixels) < 1:
            raise ValueError("a whole number >= 1")
    except (TypeError, ValueError) as e:
        raise ValueError(f"cull_mesh: min_pixels {min_pixels!r}: {e}") from None
    if visible is None:
        visible = visible_faces(mesh, Ks, poses, size, cull=cull)
    pixels = visible.get('pixels') if isinstance(visible, dict) else None
    if not torch.is_tensor(pixels) or tuple(pixels.shape) != (int(faces.shape[0]),):
        raise ValueError(f"cull_mesh: visible must be what visible_faces returned for this mesh ({int(faces.shape[0])} faces)")
    # (a face that won a pixel is usable by the rule: its indices are inside the vertices)
    return _select_faces(mesh, pts, faces, pixels.to(pts.device) >= int(min_pixels), "cull_mesh")


def write_ply(path, world):
    """``world['points']`` (M,3) float32 and ``world['colours']`` (M,3) float32 in 0..1 as a binary little-endian PLY file: per vertex
    ``x y z`` float32 and ``red green blue`` uchar, the colours by the renderer's 8-bit rule (trunc(c * 255) from the float64 product,
    clamped to 0 .. 255, NaN gives 0).  With ``world['normals']`` (M,3) float32 the vertex is ``x y z nx ny nz`` float32 and ``red green
    blue`` uchar; without, the file is what it always was.  Device tensors come to the host in one copy of 15 (27) bytes per point; CPU
    tensors work too.  With ``world['faces']`` (F,3) int32 -- ``extract_mesh``'s dict -- the file also has ``element face F`` with ``property list
    uchar int vertex_indices``, 13 bytes per face after the vertices.  Returns the path."""
    points, colours = world.get('points'), world.get('colours')
    if not torch.is_tensor(points) or not torch.is_tensor(colours) or points.dtype != torch.float32 or colours.dtype != torch.float32 \
            or points.dim() != 2 or points.shape[1] != 3 or tuple(colours.shape) != tuple(points.shape) or points.device != colours.device:
        raise ValueError("write_ply: world needs float32 points (M,3) and colours (M,3) on one device")
    M = int(points.shape[0])
    normals = world.get('normals')
    if normals is not None and (not torch.is_tensor(normals) or normals.dtype != torch.float32 or tuple(normals.shape) != (M, 3)
                                or normals.device != points.device):
        raise ValueError("write_ply: world['normals'] must be float32 (M,3) on the points' device")
    faces = world.get('faces')
    if faces is not None and (not torch.is_tensor(faces) or faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3):
        raise ValueError("write_ply: world['faces'] must be int32 (F,3)")
    rgb = torch.nan_to_num(colours.detach().double() * 255.0, nan=0.0).clamp(0.0, 255.0).to(torch.uint8)
    floats = [points] if normals is None else [points, normals]
    rows = torch.cat([t.detach().contiguous().view(torch.uint8).reshape(M, 12) for t in floats] + [rgb], dim=1).cpu().numpy()   # the one copy
    header = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {M}\n" + "property float x\nproperty float y\nproperty float z\n"
              + ("" if normals is None else "property float nx\nproperty float ny\nproperty float nz\n") +
              "property uchar red\nproperty uchar green\nproperty uchar blue\n" +
              ("" if faces is None else f"element face {int(faces.shape[0])}\nproperty list uchar int vertex_indices\n") + "end_header\n")
    if np.little_endian is False:                                                      # (the float bytes above are the host's)
        raise ValueError("write_ply: a big-endian host")
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        f.write(rows.tobytes())
        if faces is not None:                                                          # per face: the count 3 as uchar, three int32
            lists = np.empty(int(faces.shape[0]), dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
            lists['n'], lists['v'] = 3, faces.detach().cpu().numpy()
            f.write(lists.tobytes())
    return path


_PLY_FLOAT, _PLY_UCHAR = ('float', 'float32'), ('uchar', 'uint8')
_PLY_COUNT = {'uchar': 'u1', 'uint8': 'u1', 'int': '<i4', 'int32': '<i4'}
_PLY_INDEX = {'int': '<i4', 'int32': '<i4', 'uint': '<u4', 'uint32': '<u4'}


def read_ply(path, device='cpu'):
    """The inverse of ``write_ply``: a PLY file, binary little-endian or ASCII, whose ``vertex`` element has ``x y z`` float, optionally
    ``nx ny nz`` float and optionally ``red green blue`` uchar (in any order), and whose optional ``face`` element is one list property of
    ``uchar`` or ``int`` counts over ``int`` or ``uint`` indices, TRIANGLES only.  Anything else -- another format, element, property or
    type, a face that is not a triangle, an index beyond int32, a short file -- raises ``ValueError`` naming the line (of the header, or
    of an ASCII body; the element's row in a binary body).  Host code, NumPy.  Returns a world dict on ``device``: ``points`` (M,3)
    float32, ``colours`` (M,3) float32 = uchar / 255 (zeros without them), ``normals`` when the file has them, ``faces`` (F,3) int32 when
    it has a face element, ``kf_index`` / ``seg_ids`` = -1 and ``offsets`` = [0, M]: ``write_ply``, ``sample_mesh``, ``mesh_distance``
    and ``map_distance`` accept it as it is."""
    with open(path, 'rb') as f:
        data = f.read()
    end = data.find(b"end_header")
    stop = data.find(b"\n", end) if end >= 0 else -1
    if end < 0 or stop < 0:
        raise ValueError(f"read_ply: {path}: no end_header line")
    try:
        lines = data[:stop].decode('ascii').split("\n")
    except UnicodeDecodeError as e:
        raise ValueError(f"read_ply: {path}: the header is not ASCII: {e}") from None
    body = data[stop + 1:]
    bad = lambda no, why: ValueError(f"read_ply: {path}, line {no}: {why}")
    if lines[0].strip() != "ply":
        raise bad(1, f"{lines[0]!r} is not 'ply'")
    fmt, elements = None, []
    for no, line in enumerate(lines[1:], start=2):
        words = line.split()
        if not words or words[0] in ("comment", "obj_info", "end_header"):
            continue
        if words[0] == "format":
            if words[1:] not in (["binary_little_endian", "1.0"], ["ascii", "1.0"]) or fmt is not None:
                raise bad(no, f"{line!r}: the format must be given once, binary_little_endian 1.0 or ascii 1.0")
            fmt = words[1]
        elif words[0] == "element":
            if fmt is None or len(words) != 3 or not words[2].isdigit() or words[1] != ("vertex", "face")[min(len(elements), 1)] or len(elements) > 1:
                raise bad(no, f"{line!r}: the elements are 'vertex N' and then, optionally, 'face F', after the format")
            elements.append(dict(name=words[1], count=int(words[2]), props=[], line=no))
        elif words[0] == "property" and elements:
            el = elements[-1]
            if el['name'] == "vertex":
                kind = 'f' if len(words) == 3 and words[1] in _PLY_FLOAT and words[2] in ('x', 'y', 'z', 'nx', 'ny', 'nz') else \
                    'u' if len(words) == 3 and words[1] in _PLY_UCHAR and words[2] in ('red', 'green', 'blue') else None
                if kind is None or words[2] in [p[0] for p in el['props']]:
                    raise bad(no, f"{line!r}: a vertex has x y z (float), nx ny nz (float) and red green blue (uchar), each once")
                el['props'].append((words[2], '<f4' if kind == 'f' else 'u1'))
            else:
                if len(words) != 5 or words[1] != "list" or words[2] not in _PLY_COUNT or words[3] not in _PLY_INDEX \
                        or words[4] not in ("vertex_indices", "vertex_index") or el['props']:
                    raise bad(no, f"{line!r}: a face is one 'property list uchar|int int|uint vertex_indices'")
                el['props'].append((_PLY_COUNT[words[2]], _PLY_INDEX[words[3]]))
        else:
            raise bad(no, f"{line!r}: not a line of a PLY header this reader takes")
    if not elements:
        raise bad(len(lines), "no vertex element")
    vertex = elements[0]
    names = [p[0] for p in vertex['props']]
    for group in (('x', 'y', 'z'), ('nx', 'ny', 'nz'), ('red', 'green', 'blue')):
        have = [k in names for k in group]
        if (group[0] == 'x' and not all(have)) or (any(have) and not all(have)):
            raise bad(vertex['line'], f"the vertex has {names}: {' '.join(group)} come together" + (" and x y z are required" if group[0] == 'x' else ""))
    face = elements[1] if len(elements) > 1 else None
    if face is not None and not face['props']:
        raise bad(face['line'], "the face element has no property")
    M, F = vertex['count'], face['count'] if face else 0
    vdt = np.dtype(vertex['props'])
    tri = None
    if fmt == "binary_little_endian":
        fdt = np.dtype([('n', face['props'][0][0]), ('v', face['props'][0][1], (3,))]) if face else None
        if len(body) < M * vdt.itemsize:
            raise bad(len(lines) + 1, f"the body holds {len(body)} bytes, {M} vertices need {M * vdt.itemsize}")
        rows = np.frombuffer(body, dtype=vdt, count=M)
        if face:
            rest = body[M * vdt.itemsize:]
            whole = np.frombuffer(rest, dtype=fdt, count=min(F, len(rest) // fdt.itemsize))
            odd = np.nonzero(whole['n'] != 3)[0]
            if len(odd):
                raise bad(len(lines) + 1, f"face {int(odd[0])} has {int(whole['n'][odd[0]])} vertices: triangles only")
            if len(whole) < F or len(rest) != F * fdt.itemsize:
                raise bad(len(lines) + 1, f"{len(rest)} bytes after the vertices, {F} triangles need {F * fdt.itemsize}")
            tri = whole['v'].astype(np.int64)
    else:
        first = len(lines) + 1                                                          # the file's line number of the body's first line
        numbered = [(first + j, t) for j, t in enumerate(body.decode('ascii', errors='replace').split("\n")) if t.strip()]
        if len(numbered) != M + F:
            raise bad(numbered[-1][0] if numbered else first, f"the body has {len(numbered)} lines, {M} vertices and {F} faces need {M + F}")
        at, text = [a for a, _ in numbered], [t for _, t in numbered]
        rows = np.zeros(M, dtype=vdt)
        for r in range(M):
            words = text[r].split()
            try:
                if len(words) != len(names):
                    raise ValueError(f"{len(words)} numbers for {len(names)} properties")
                for (name, kind), w in zip(vertex['props'], words):
                    rows[name][r] = float(w) if kind == '<f4' else int(w)
                    if kind == 'u1' and not 0 <= int(w) <= 255:
                        raise ValueError(f"{w} is no uchar")
            except (ValueError, OverflowError) as e:
                raise bad(at[r], f"{text[r]!r}: {e}") from None
        if face:
            tri = np.zeros((F, 3), np.int64)
            for r in range(F):
                words = text[M + r].split()
                try:
                    nums = [int(w) for w in words]
                    if not nums or nums[0] != len(nums) - 1:
                        raise ValueError("a list is its length and then that many indices")
                    if nums[0] != 3:
                        raise ValueError(f"a face of {nums[0]} vertices: triangles only")
                    tri[r] = nums[1:]
                except ValueError as e:
                    raise bad(at[M + r], f"{text[M + r]!r}: {e}") from None
    if tri is not None and len(tri) and (tri.min() < -2 ** 31 or tri.max() > 2 ** 31 - 1):
        raise bad(len(lines) + 1, f"a face index {int(tri.max())} is beyond int32")
    stack = lambda keys, dtype: torch.from_numpy(np.ascontiguousarray(np.stack([rows[k] for k in keys], axis=1).astype(dtype))).to(device)
    out = dict(points=stack(('x', 'y', 'z'), np.float32))
    if 'red' in names:
        out['colours'] = torch.from_numpy(np.stack([rows[k] for k in ('red', 'green', 'blue')], axis=1).astype(np.float32) / np.float32(255.0)).to(device)
    else:
        out['colours'] = torch.zeros(M, 3, dtype=torch.float32, device=device)
    if 'nx' in names:
        out['normals'] = stack(('nx', 'ny', 'nz'), np.float32)
    if face is not None:
        out['faces'] = torch.from_numpy(tri.astype(np.int32).reshape(F, 3)).to(device)
    none = torch.full((M,), -1, dtype=torch.int32, device=device)
    out.update(kf_index=none, seg_ids=none.clone(), offsets=np.array([0, M], dtype=np.int64))
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
