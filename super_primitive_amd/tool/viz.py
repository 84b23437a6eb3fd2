"""The two array routines of the reference's ``tool/viz.py`` that the viewers call, on the device (csrc/sp_views.hip; no open3d, cv2 or
matplotlib is imported):

``render_pcd``         ``tool/viz.py:180-190``: camera-frame points splatted into an (H,W,3) uint8 image, the highest index winning a pixel;
                       with ``depth_buffer=True`` the nearest point wins instead.
``depth_image_lift``   ``tool/viz.py:30-51``: a depth image lifted into a coloured point cloud (Open3D's ``create_from_depth_image`` with
                       ``depth_scale=1, depth_trunc=100, stride=1``, then ``transform(T)``).  Returns tensors, not an Open3D object.
``lift_depth_images``  the batched lift without a synchronisation.
``render_views``       the call under ``render_pcd`` and ``odometery.results.render_map``: V posed views of one point set per launch;
                       with ``radii`` every point is a square footprint (``sp_render_splats``): no holes where the map is sparser than the view;
                       with ``normals`` on top an oriented surfel (``sp_render_surfels``): a slanted surface renders at its true depth.
``image_metrics``      rendered views against real images: exact integer sums per view (``sp_image_metrics``).
``keyframe_normals``   the surface normal of every row of an ``sp_map_points`` launch, from the same records (``sp_map_normals``).
``keyframe_depths``    what each keyframe claims to see: its own depth image and segment map, from its table (``sp_keyframe_depths``).
``map_consistency``    every point against V depth images: agree / in front / behind counts per point (``sp_map_consistency``).
``fuse_points``        one averaged point per occupied voxel of a point set (``sp_map_fuse``).
``cloud_grid``         a point cloud prepared for neighbour queries at one radius (``sp_cloud_grid_build``).
``nearest_points``     per query point the nearest point of such a cloud, its distance and the count within the radius (``sp_cloud_grid_nearest``).
``nearest_k``          per query point its k nearest points of such a cloud within the radius, sorted (``sp_cloud_grid_knn``).
``cloud_normals``      a normal and a surface variation per point of a cloud that has none, from its k nearest points (``sp_cloud_normals``).
``tsdf_integrate``     depth images fused into a dense signed-distance volume, in place (``sp_tsdf_integrate``).
``tsdf_mesh``          the volume's zero level set as an indexed triangle mesh: a counting call, one host read, a filling call (``sp_tsdf_mesh``).
``tsdf_raycast``       the volume seen from V cameras: depth, world normals, colour and cell index per pixel, one ray each (``sp_tsdf_raycast``).
``mesh_faces``         one record per face of a triangle mesh: state, area, unit normal, and the summary counts (``sp_mesh_faces``).
``mesh_sample``        an area-uniform, seeded cloud with normals from those records: a counting call, one host read, a filling call
                       (``sp_mesh_sample``).
``mesh_render``       the mesh seen from V cameras: depth, world normals, interpolated colour and winning face per pixel, rasterised
                       through the depth buffer (``sp_mesh_render``).
``register_clouds``    the similarity that moves a query cloud onto such a cloud, by Gauss-Newton ICP on the device (``sp_cloud_register``).

Argument errors raise ``ValueError`` before anything is launched."""
from __future__ import annotations

import torch

from .. import _lib

Z_MIN = 1e-6          # the depth buffer's near bound: the project's figure in sp_depth_splat


def _on_device(*tensors):
    for t in tensors:
        if t is not None and not torch.is_tensor(t):
            raise ValueError(f"super_primitive_amd.tool.viz takes cuda tensors, got {type(t).__name__}")
    try:
        _lib.require_device(*tensors)
    except RuntimeError as e:
        raise ValueError(str(e)) from None


def _f32(t, shape, what):
    """``t`` as a contiguous float32 tensor of ``shape`` (None: any size there); points, colours and depths must be float32 already."""
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError(f"{what} must have shape {tuple('*' if s is None else s for s in shape)}, got {tuple(t.shape)}")
    return t.detach().contiguous()


def _cameras(K, n, what):
    """(n,9) float32 from (3,3) (shared by all) or (n,3,3) of any floating type."""
    if not K.is_floating_point() or tuple(K.shape) not in ((3, 3), (n, 3, 3)):
        raise ValueError(f"{what} must be floating (3,3) or ({n},3,3), got {K.dtype} {tuple(K.shape)}")
    return K.detach().float().reshape(-1, 9).expand(n, 9).contiguous()


def _poses(T, n, what):
    if not T.is_floating_point() or tuple(T.shape) not in ((4, 4), (n, 4, 4)):
        raise ValueError(f"{what} must be floating (4,4) or ({n},4,4), got {T.dtype} {tuple(T.shape)}")
    return T.detach().float().reshape(-1, 16).expand(n, 16).contiguous()


def _size(H, W):
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"image size {H}x{W}")
    return H, W


def _views(Ks, poses, V):
    """The (V,25) contiguous float32 tensor of V ``SpView`` records: K row major, then the camera-to-world pose."""
    return torch.cat((_cameras(Ks, V, "Ks"), _poses(poses, V, "poses")), dim=1).contiguous()


def _z_min(z_min):
    if not float(z_min) >= 0.0:
        raise ValueError(f"z_min {z_min}")


def _limits(what, V, H, W, Q=0, views="views"):
    """The map kernels' limits: ids and pixels are 32-bit, a grid dimension 16-bit."""
    if Q > 2 ** 31 - 2 or V > 65535 or V * H * W >= 2 ** 31:
        raise ValueError(f"{what}: {f'{Q} points, ' if Q else ''}{V} {views} of {H}x{W} are beyond the kernel's limits")


def _view_count(poses, what=None):
    """V of ``poses`` (V,4,4), the first check of every launcher over a view set; with ``what``, V = 0 is that launcher's error (a
    launcher that takes points reports an empty set of either in one message of its own, once it has seen the points)."""
    if poses.dim() != 3:
        raise ValueError(f"poses must be (V,4,4), got {tuple(poses.shape)}")
    V = int(poses.shape[0])
    if what and V == 0:
        raise ValueError(f"{what}: poses of no views")
    return V


def _view_set(Ks, poses, V, H, W):
    """The rest of that prologue, where nothing comes between its two checks: the image size is positive, and ``Ks`` and ``poses`` make
    V ``SpView`` records.  Returns (views, H, W)."""
    H, W = _size(H, W)
    return _views(Ks, poses, V), H, W


_VIEW_IMAGES = dict(depth=((), torch.float32), normals=((3,), torch.float32), image=((3,), torch.uint8), index=((), torch.int32))


def _view_images(V, H, W, device, **wanted):
    """The wanted of the view images as a dict, uninitialised, in the order given: ``depth`` (V,H,W) float32, ``normals`` (V,H,W,3)
    float32, ``image`` (V,H,W,3) uint8, ``index`` (V,H,W) int32."""
    return {k: torch.empty(V, H, W, *_VIEW_IMAGES[k][0], dtype=_VIEW_IMAGES[k][1], device=device) for k, want in wanted.items() if want}


def render_views(points, colours, Ks, poses, H, W, depth_buffer=False, z_min=Z_MIN, image=True, depth=True, index=True, radii=None,
                 max_px=8, normals=None, cull=False):
    """ONE ``sp_render_views`` launch (include/sp_hip.h has the arithmetic): ``points`` (Q,3) float32 in the world, ``colours`` (Q,3)
    float32 in 0..1 (None allowed without ``image``), ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4) camera-to-world.  Returns the requested
    of ``image`` (V,H,W,3) uint8, ``depth`` (V,H,W) float32 (0 where nothing landed) and ``index`` (V,H,W) int32 (-1 there) as a dict.
    ``radii`` (Q,) float32 in world units: ONE ``sp_render_splats`` launch instead -- every point covers the pixels its square footprint
    of that half side touches, at most ``max_px`` (0 .. 16) pixels to either side, through the depth buffer (``depth_buffer`` must be
    true).  ``normals`` (Q,3) float32 in the frame of the points (``radii`` required): ONE ``sp_render_surfels`` launch -- the depth of
    every covered pixel is taken on the point's tangent plane, clamped to ``z -+ 2 radius``; a zero or non-finite normal is a flat
    footprint; ``cull=True`` drops surfels seen from behind.  No synchronisation."""
    _on_device(points, colours, Ks, poses, radii, normals)
    H, W = _size(H, W)
    V = _view_count(poses)
    pts = _f32(points, (None, 3), "points")
    Q = int(pts.shape[0])
    if Q == 0 or V == 0:
        raise ValueError(f"render_views: {Q} points into {V} views")
    if image and colours is None:
        raise ValueError("render_views: an image needs colours")
    cols = None if colours is None else _f32(colours, (Q, 3), "colours")
    views = _views(Ks, poses, V)
    _z_min(z_min)
    rad = None
    if radii is not None:
        if not depth_buffer:
            raise ValueError("render_views: radii need depth_buffer=True (footprints go through the depth buffer)")
        rad = _f32(radii, (Q,), "radii")
        if int(max_px) != max_px or not 0 <= int(max_px) <= 16:
            raise ValueError(f"render_views: max_px {max_px} (0 .. 16)")
    nrm = None
    if normals is not None:
        if rad is None:
            raise ValueError("render_views: normals need radii (a surfel is an oriented footprint) and depth_buffer=True")
        nrm = _f32(normals, (Q, 3), "normals")
    elif cull:
        raise ValueError("render_views: cull needs normals")
    _limits("render_views", V, H, W, Q)
    lib = _lib.load()
    keys = torch.empty(V * H * W, dtype=torch.int64, device=pts.device)
    out = _view_images(V, H, W, pts.device, image=image, depth=depth, index=index)
    if nrm is not None:
        _lib.check(lib.sp_render_surfels(_lib.ptr(pts), _lib.ptr(cols), _lib.ptr(nrm), Q, _lib.ptr(views), V, H, W, float(z_min), _lib.ptr(rad),
                                         int(max_px), 1 if cull else 0, _lib.ptr(keys), _lib.ptr(out.get('image')), _lib.ptr(out.get('depth')),
                                         _lib.ptr(out.get('index')), _lib.stream_ptr()), "sp_render_surfels")
        return out
    if rad is not None:
        _lib.check(lib.sp_render_splats(_lib.ptr(pts), _lib.ptr(cols), Q, _lib.ptr(views), V, H, W, float(z_min), _lib.ptr(rad), int(max_px),
                                        _lib.ptr(keys), _lib.ptr(out.get('image')), _lib.ptr(out.get('depth')), _lib.ptr(out.get('index')),
                                        _lib.stream_ptr()), "sp_render_splats")
        return out
    _lib.check(lib.sp_render_views(_lib.ptr(pts), _lib.ptr(cols), Q, _lib.ptr(views), V, H, W, 1 if depth_buffer else 0, float(z_min),
                                   _lib.ptr(keys), _lib.ptr(out.get('image')), _lib.ptr(out.get('depth')), _lib.ptr(out.get('index')),
                                   _lib.stream_ptr()), "sp_render_views")
    return out


def image_metrics(rendered, target, index):
    """ONE ``sp_image_metrics`` launch: ``rendered`` (V,H,W,3) uint8 and ``index`` (V,H,W) int32 as ``render_views`` returns them,
    ``target`` (V,3,H,W) float32 in 0..1 (the project's planar layout), converted to 0 .. 255 by the renderer's own rule.  Returns (V,3)
    int64 on the device: per view n, sum |a - b| and sum (a - b)^2 over the pixels with ``index >= 0`` and their three channels -- exact
    integers.  No synchronisation."""
    _on_device(rendered, target, index)
    if rendered.dtype != torch.uint8 or rendered.dim() != 4 or rendered.shape[3] != 3 or 0 in rendered.shape:
        raise ValueError(f"rendered must be uint8 (V,H,W,3), got {rendered.dtype} {tuple(rendered.shape)}")
    V, H, W = (int(s) for s in rendered.shape[:3])
    if index.dtype != torch.int32 or tuple(index.shape) != (V, H, W):
        raise ValueError(f"index must be int32 {(V, H, W)}, got {index.dtype} {tuple(index.shape)}")
    tgt = _f32(target, (V, 3, H, W), "target")
    _limits("image_metrics", V, H, W)
    lib = _lib.load()
    img, idx = rendered.contiguous(), index.contiguous()
    out = torch.empty(V, 3, dtype=torch.int64, device=img.device)
    _lib.check(lib.sp_image_metrics(_lib.ptr(img), _lib.ptr(tgt), _lib.ptr(idx), V, H, W, _lib.ptr(out), _lib.stream_ptr()), "sp_image_metrics")
    return out


def render_pcd(points_3d, points_colour, K, H, W, *, depth_buffer=False, return_maps=False):
    """``tool/viz.py:180-190``: ``points_3d`` (Q,3) float32 in the CAMERA frame, ``points_colour`` (Q,3) float32 in 0..1, ``K`` (3,3).
    Returns the (H,W,3) uint8 image; with ``return_maps`` also the (H,W) float32 depth and (H,W) int32 point index of every pixel.
    The default is the reference: no test on z, the highest index wins a pixel (colours beyond 0..1 are clamped where the reference's
    ``astype(uint8)`` wraps).  ``depth_buffer=True``: only z > 1e-6, the nearest point wins."""
    _on_device(points_3d, points_colour, K)
    if tuple(K.shape) != (3, 3):
        raise ValueError(f"K must be (3,3), got {tuple(K.shape)}")
    eye = torch.eye(4, dtype=torch.float32, device=points_3d.device)[None]
    out = render_views(points_3d, points_colour, K, eye, H, W, depth_buffer=depth_buffer, depth=return_maps, index=return_maps)
    return (out['image'][0], out['depth'][0], out['index'][0]) if return_maps else out['image'][0]


def lift_depth_images(depths, Ks, poses=None, images=None, depth_trunc=100.0):
    """ONE ``sp_depth_lift`` call: ``depths`` (B,H,W) float32, ``Ks`` (B,3,3) or (3,3), ``poses`` (B,4,4) camera-to-world or None,
    ``images`` (B,3,H,W) float32 or None.  A pixel is valid iff 0 < d <= depth_trunc.  Returns the CAPACITY buffers ``points`` (B H W, 3),
    ``colours`` (B H W, 3) (with images), ``pixel`` (B H W,) int32 = r W + c, and ``counts`` (B,) int32, ``offsets`` (B+1,) int64 on the
    device: row offsets[b] + k is the k-th valid pixel of image b in row-major order; rows from offsets[B] on are uninitialised.
    No synchronisation."""
    _on_device(depths, Ks, poses, images)
    d = _f32(depths, (None, None, None), "depths")
    B, H, W = (int(s) for s in d.shape)
    if B == 0 or H == 0 or W == 0:
        raise ValueError(f"depths {tuple(d.shape)}")
    K = _cameras(Ks, B, "Ks")
    T = None if poses is None else _poses(poses, B, "poses")
    img = None if images is None else _f32(images, (B, 3, H, W), "images")
    if not float(depth_trunc) > 0.0:
        raise ValueError(f"depth_trunc {depth_trunc}")
    lib = _lib.load()
    n_blocks = lib.sp_depth_lift_blocks(B, H, W)
    if n_blocks < 0:
        raise ValueError(f"lift_depth_images: {B} images of {H}x{W} are beyond the kernel's limits")
    dev, cap = d.device, B * H * W
    scratch = torch.empty(n_blocks, dtype=torch.int32, device=dev)
    out = dict(points=torch.empty(cap, 3, dtype=torch.float32, device=dev), pixel=torch.empty(cap, dtype=torch.int32, device=dev),
               counts=torch.empty(B, dtype=torch.int32, device=dev), offsets=torch.empty(B + 1, dtype=torch.int64, device=dev))
    if img is not None:
        out['colours'] = torch.empty(cap, 3, dtype=torch.float32, device=dev)
    _lib.check(lib.sp_depth_lift(_lib.ptr(d), _lib.ptr(K), _lib.ptr(T), _lib.ptr(img), B, H, W, float(depth_trunc), _lib.ptr(scratch),
                                 _lib.ptr(out['points']), _lib.ptr(out.get('colours')), _lib.ptr(out['pixel']), _lib.ptr(out['counts']),
                                 _lib.ptr(out['offsets']), _lib.stream_ptr()), "sp_depth_lift")
    return out


def depth_image_lift(depth, K, image=None, mask=None, T=None, depth_trunc=100.0):
    """``tool/viz.py:30-51`` for one image: ``depth`` (H,W) float32, ``K`` (3,3), ``image`` (3,H,W) float32 (the project's planar layout,
    already in 0..1), ``T`` (4,4) camera-to-world.  ``mask``: as in the reference, a boolean over the COMPACTED rows (one entry per valid
    pixel, row-major), applied to points, colours and pixel.  Returns ``dict(points (n,3), colours (n,3) or None, pixel (n,))`` trimmed to
    the valid count: reading that count is the ONE synchronisation of this call (``lift_depth_images`` has none)."""
    _on_device(depth, K, image, mask, T)
    if depth.dim() != 2:
        raise ValueError(f"depth must be (H,W), got {tuple(depth.shape)}")
    if image is not None and image.dim() != 3:
        raise ValueError(f"image must be (3,H,W), got {tuple(image.shape)}")
    if T is not None and tuple(T.shape) != (4, 4):
        raise ValueError(f"T must be (4,4), got {tuple(T.shape)}")
    if mask is not None and mask.dtype != torch.bool:
        raise ValueError(f"mask must be boolean, got {mask.dtype}")
    out = lift_depth_images(depth[None], K, None if T is None else T[None], None if image is None else image[None], depth_trunc)
    n = int(out['offsets'][1])                                               # the one host read
    res = dict(points=out['points'][:n], colours=out['colours'][:n] if image is not None else None, pixel=out['pixel'][:n])
    if mask is not None:
        mask = mask.reshape(-1)
        if mask.numel() != n:
            raise ValueError(f"mask has {mask.numel()} entries for {n} valid pixels")
        res = {k: (None if v is None else v[mask]) for k, v in res.items()}
    return res


_BLOCK = 256          # rows per workgroup of the keyframe walk (sp_map_points, sp_keyframe_depths): SP_BLOCK


def keyframe_records(what, kfs, klds, stride=1, poses=None, align_index=None):
    """The ``SpMapKeyframe`` records of one keyframe walk over every ``stride``-th table point: tables, log-depths and the ``first_block``
    / ``out_offset`` accounting.  ``poses`` ((n,4,4) contiguous float32): also the keyframes' images and cameras, these poses and
    ``align_index`` (n integers, default -1), which sp_map_points reads on top.  Raises ``ValueError`` as ``what`` before any pointer is
    taken.  Returns (the records on the device, what they point at -- alive until the launch is queued --, the (n+1) row offsets, the workgroups)."""
    from ..segment_table import table_of
    rows = []                                              # per keyframe: table, log-depths and, with poses, image and K
    for k, (kf, kld) in enumerate(zip(kfs, klds)):
        tab = table_of(kf)                                 # (raises ValueError for a keyframe without segment pixels)
        cam = [] if poses is None else [kf.image[:3].detach().contiguous().float(), kf.K.detach().contiguous().float()]
        if cam and (tuple(cam[0].shape) != (3, tab.H, tab.W) or cam[1].numel() != 9 or poses[k].numel() != 16):
            raise ValueError(f"{what}: keyframe {k}: image {tuple(cam[0].shape)} against segments of {tab.H}x{tab.W}, K of {cam[1].numel()}, pose of {poses[k].numel()}")
        rows.append((tab, kld.detach().contiguous().float(), *cam))
        if rows[-1][1].numel() != tab.N:
            raise ValueError(f"{what}: keyframe {k}: {rows[-1][1].numel()} log-depths for {tab.N} segments")
    recs, offsets, block = (_lib.SpMapKeyframe * len(rows))(), [0], 0
    for k, (r, (tab, kld_c, *cam)) in enumerate(zip(recs, rows)):
        r.pix, r.baseL, r.seg_off, r.kp_L, r.kld = tab.pix.data_ptr(), tab.baseL.data_ptr(), tab.seg_off.data_ptr(), tab.kp_L.data_ptr(), kld_c.data_ptr()
        if cam:
            r.image, r.K, r.pose = cam[0].data_ptr(), cam[1].data_ptr(), poses[k].data_ptr()
        r.N, r.P, r.H, r.W = tab.N, tab.P, tab.H, tab.W
        q = (tab.P + stride - 1) // stride
        r.out_offset, r.align, r.first_block = offsets[k], -1 if align_index is None else int(align_index[k]), block
        offsets.append(offsets[k] + q)
        block += (q + _BLOCK - 1) // _BLOCK
    return torch.frombuffer(bytearray(bytes(recs)), dtype=torch.uint8).to(rows[0][1].device), [poses, rows], offsets, block


def keyframe_normals(recs_d, n, blocks, stride, total, record=None):
    """ONE ``sp_map_normals`` launch (include/sp_hip.h has the arithmetic) over the records of ``keyframe_records(..., poses=...)``:
    ``recs_d`` and ``blocks`` as it returned them for ``n`` keyframes at ``stride``, ``total`` its last row offset, ``record`` the (S,32)
    float64 alignment records or None -- the arguments of the ``sp_map_points`` launch whose rows these normals belong to.  What the
    records point at must still be alive.  Returns (total,3) float32 on the device: unit normals in the world that face their
    keyframe's camera, (0, 0, 0) where the table gives none.  No synchronisation."""
    lib = _lib.load()
    normals = torch.empty(total, 3, dtype=torch.float32, device=recs_d.device)
    _lib.check(lib.sp_map_normals(_lib.ptr(recs_d), n, blocks, stride, _lib.ptr(record), 0 if record is None else int(record.shape[0]),
                                  _lib.ptr(normals), total, _lib.stream_ptr()), "sp_map_normals")
    return normals


def keyframe_depths(kfs, klds):
    """ONE ``sp_keyframe_depths`` call (include/sp_hip.h): what each keyframe claims to see, straight from its segment table -- per
    pixel the nearest table point's depth ``exp(baseL + (kld[n] - kp_L[n]))`` (the depth ``odometery.results.keyframe_points`` gives
    the same point, bit for bit) and its segment.  ``kfs``: keyframes with segments, all of ONE size; ``klds``: their keypoint
    log-depths.  Returns ``dict(depth (n,H,W) float32 -- 0 where no point lies --, seg (n,H,W) int32 -- -1 there)``.  Raises
    ``ValueError`` for keyframes of differing sizes or without segment pixels.  No synchronisation beyond the table builds."""
    from ..segment_table import table_of
    n = len(kfs)
    if n == 0 or len(klds) != n:
        raise ValueError(f"keyframe_depths: {n} keyframes, {len(klds)} log-depth vectors")
    _on_device(*klds)
    sizes = [(tab.H, tab.W) for tab in map(table_of, kfs)]                   # (raises ValueError for a keyframe without segment pixels)
    H, W = sizes[0]
    if sizes.count(sizes[0]) != n:
        raise ValueError(f"keyframe_depths: keyframes of differing sizes {sorted(set(sizes))}")
    _limits("keyframe_depths", n, H, W, views="keyframes")
    recs_d, keep, _, blocks = keyframe_records("keyframe_depths", kfs, klds)   # (image, pose, align and out_offset are not read)
    lib = _lib.load()
    dev = recs_d.device
    keys = torch.empty(n * H * W, dtype=torch.int64, device=dev)
    out = dict(depth=torch.empty(n, H, W, dtype=torch.float32, device=dev), seg=torch.empty(n, H, W, dtype=torch.int32, device=dev))
    _lib.check(lib.sp_keyframe_depths(_lib.ptr(recs_d), n, blocks, H, W, _lib.ptr(keys), _lib.ptr(out['depth']), _lib.ptr(out['seg']),
                                      _lib.stream_ptr()), "sp_keyframe_depths")
    return out


def _i32(t, n, what):
    if t.dtype != torch.int32 or tuple(t.shape) != (n,):
        raise ValueError(f"{what} must be int32 ({n},), got {t.dtype} {tuple(t.shape)}")
    return t.detach().contiguous()


def map_consistency(points, Ks, poses, depths, owner=None, view_owner=None, tol=0.05, window=1, z_min=Z_MIN):
    """ONE ``sp_map_consistency`` launch (include/sp_hip.h has the rule): ``points`` (Q,3) float32 in the frame of ``poses`` (V,4,4)
    camera-to-world, ``Ks`` (V,3,3) or (3,3), ``depths`` (V,H,W) float32 -- what each view claims to see (``keyframe_depths``) or ground
    truth.  A point agrees with a view when a valid depth within ``window`` (0 .. 2) pixels of its projection is within ``tol``
    (relative, 0 <= tol < 1) of its own; it is in front when it is nearer than all of them, else behind.  ``owner`` (Q,) and
    ``view_owner`` (V,) int32: a point is not tested against a view of its own owner (>= 0).  Returns (Q,3) int32 on the device: per
    point the number of views it agrees with, is in front of, is behind.  No synchronisation."""
    _on_device(points, Ks, poses, depths, owner, view_owner)
    V = _view_count(poses)
    pts = _f32(points, (None, 3), "points")
    Q = int(pts.shape[0])
    if Q == 0 or V == 0:
        raise ValueError(f"map_consistency: {Q} points against {V} views")
    d = _f32(depths, (V, None, None), "depths")
    views, H, W = _view_set(Ks, poses, V, d.shape[1], d.shape[2])
    own = None if owner is None else _i32(owner, Q, "owner")
    vown = None if view_owner is None else _i32(view_owner, V, "view_owner")
    if not 0.0 <= float(tol) < 1.0:
        raise ValueError(f"map_consistency: tol {tol} (0 <= tol < 1)")
    if int(window) != window or not 0 <= int(window) <= 2:
        raise ValueError(f"map_consistency: window {window} (0 .. 2)")
    _z_min(z_min)
    _limits("map_consistency", V, H, W, Q)
    lib = _lib.load()
    counts = torch.empty(Q, 3, dtype=torch.int32, device=pts.device)
    _lib.check(lib.sp_map_consistency(_lib.ptr(pts), _lib.ptr(own), Q, _lib.ptr(views), _lib.ptr(vown), V, _lib.ptr(d), H, W, float(tol),
                                      int(window), float(z_min), _lib.ptr(counts), _lib.stream_ptr()), "sp_map_consistency")
    return counts


def fuse_points(points, colours=None, voxel=0.05, origin=None):
    """ONE ``sp_map_fuse`` call (include/sp_hip.h has the rule): ``points`` (Q,3) float32, ``colours`` (Q,3) float32 or None, ``voxel``
    the voxel's side (a finite float32 > 0), ``origin`` three finite numbers (default: 0, 0, 0).  The points of one voxel become their
    mean -- positions quantised to 1/65536 of a voxel, colours to 8 bits, so the sums are integers and two runs give the same bits --;
    the voxels come in the order of their first input row.  Points with a non-finite coordinate, or beyond 2^20 voxels from the origin,
    are dropped.  Returns the CAPACITY buffers ``points`` (Q,3), ``colours`` (Q,3) or None, ``count`` (Q,) int32 (members per fused
    point), ``first`` (Q,) int32 (its lowest input row; pre-filled with 2^31 - 1, so rows beyond ``n`` sort after every real row),
    ``label`` (Q,) int32 (the fused row of every input row, -1 for a dropped one) and ``n`` (0-dim int64 on the device: the number of
    fused points; rows from ``n`` on are uninitialised).  No synchronisation."""
    _on_device(points, colours)
    pts = _f32(points, (None, 3), "points")
    Q = int(pts.shape[0])
    if Q == 0:
        raise ValueError("fuse_points: no points")
    cols = None if colours is None else _f32(colours, (Q, 3), "colours")
    try:
        vox = float(torch.tensor(float(voxel), dtype=torch.float32))           # the float32 the kernel divides by
        org = [0.0, 0.0, 0.0] if origin is None else [float(o) for o in torch.as_tensor(origin, dtype=torch.float64).reshape(-1).float().tolist()]
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"fuse_points: voxel {voxel!r}, origin {origin!r}: {e}") from None
    if not (vox > 0.0 and vox < float("inf")):
        raise ValueError(f"fuse_points: voxel {voxel} (a finite float32 > 0)")
    if len(org) != 3 or not all(abs(o) < float("inf") for o in org):
        raise ValueError(f"fuse_points: origin {origin} (three finite float32 numbers)")
    if Q > _lib.SP_MAP_FUSE_MAX_POINTS:
        raise ValueError(f"fuse_points: {Q} points are beyond the kernel's limit of {_lib.SP_MAP_FUSE_MAX_POINTS}")
    lib = _lib.load()
    units = lib.sp_map_fuse_scratch_units(Q)
    if units < 0:
        raise ValueError(f"fuse_points: {Q} points are beyond the kernel's limits")
    dev = pts.device
    scratch = torch.empty(units, 8, dtype=torch.int64, device=dev)
    out = dict(points=torch.empty(Q, 3, dtype=torch.float32, device=dev), colours=None if cols is None else torch.empty(Q, 3, dtype=torch.float32, device=dev),
               count=torch.empty(Q, dtype=torch.int32, device=dev), first=torch.full((Q,), 2 ** 31 - 1, dtype=torch.int32, device=dev),
               label=torch.empty(Q, dtype=torch.int32, device=dev), n=torch.empty((), dtype=torch.int64, device=dev))
    _lib.check(lib.sp_map_fuse(_lib.ptr(pts), _lib.ptr(cols), Q, vox, org[0], org[1], org[2], _lib.ptr(scratch), _lib.ptr(out['points']),
                               _lib.ptr(out['colours']), _lib.ptr(out['count']), _lib.ptr(out['first']), _lib.ptr(out['label']), _lib.ptr(out['n']),
                               _lib.stream_ptr()), "sp_map_fuse")
    return out


def cloud_grid(points, radius, origin=None):
    """ONE ``sp_cloud_grid_build`` call (include/sp_hip.h has the rule): ``points`` (Q,3) float32, the REFERENCE cloud, prepared for
    ``nearest_points`` at search radius ``radius`` (a finite float32 > 0); ``origin`` three finite numbers (default: 0, 0, 0) -- points
    beyond 2^20 cells of side ``radius`` from it, or with a non-finite coordinate, are never found.  Returns the handle
    ``dict(scratch, Q, radius, origin, points)``; the points tensor is kept alive there for ``skip_self``.  No synchronisation."""
    _on_device(points)
    pts = _f32(points, (None, 3), "points")
    Q = int(pts.shape[0])
    if Q == 0:
        raise ValueError("cloud_grid: no points")
    try:
        rad = float(torch.tensor(float(radius), dtype=torch.float32))          # the float32 the kernel squares
        org = [0.0, 0.0, 0.0] if origin is None else [float(o) for o in torch.as_tensor(origin, dtype=torch.float64).reshape(-1).float().tolist()]
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"cloud_grid: radius {radius!r}, origin {origin!r}: {e}") from None
    if not (rad > 0.0 and rad < float("inf")):
        raise ValueError(f"cloud_grid: radius {radius} (a finite float32 > 0)")
    if len(org) != 3 or not all(abs(o) < float("inf") for o in org):
        raise ValueError(f"cloud_grid: origin {origin} (three finite float32 numbers)")
    if Q > _lib.SP_CLOUD_GRID_MAX_POINTS:
        raise ValueError(f"cloud_grid: {Q} points are beyond the kernel's limit of {_lib.SP_CLOUD_GRID_MAX_POINTS}")
    lib = _lib.load()
    units = lib.sp_cloud_grid_scratch_units(Q)
    if units < 0:
        raise ValueError(f"cloud_grid: {Q} points are beyond the kernel's limits")
    scratch = torch.empty(units, 8, dtype=torch.int64, device=pts.device)
    _lib.check(lib.sp_cloud_grid_build(_lib.ptr(pts), Q, rad, org[0], org[1], org[2], _lib.ptr(scratch), _lib.stream_ptr()), "sp_cloud_grid_build")
    return dict(scratch=scratch, Q=Q, radius=rad, origin=tuple(org), points=pts)


def _grid_handle(grid, what):
    """(Q, scratch) of what ``cloud_grid`` returned; ``ValueError`` for anything else, before any tensor is touched."""
    if not isinstance(grid, dict) or any(k not in grid for k in ('scratch', 'Q', 'radius', 'origin', 'points')) \
            or not torch.is_tensor(grid['scratch']) or not torch.is_tensor(grid['points']):
        raise ValueError(f"{what}: grid must be what cloud_grid returned")
    Q = int(grid['Q'])
    if not 1 <= Q <= _lib.SP_CLOUD_GRID_MAX_POINTS or int(grid['points'].shape[0]) != Q:
        raise ValueError(f"{what}: a grid of {Q} points over a cloud of {int(grid['points'].shape[0])}")
    return Q, grid['scratch']


def _grid_scratch(grid, what):
    """The library, once the handle's scratch has the size ``sp_cloud_grid_build`` wrote for its Q points (the last check: it needs the library)."""
    lib = _lib.load()
    Q, scratch = int(grid['Q']), grid['scratch']
    if scratch.dtype != torch.int64 or not scratch.is_contiguous() or scratch.numel() != 8 * lib.sp_cloud_grid_scratch_units(Q):
        raise ValueError(f"{what}: the grid's scratch ({scratch.dtype}, {scratch.numel()} elements) is not that of {Q} points")
    return lib


def nearest_points(queries, grid, skip_self=False):
    """ONE ``sp_cloud_grid_nearest`` call: per row of ``queries`` (Qa,3) float32 the nearest point of the cloud behind ``grid`` (what
    ``cloud_grid`` returned) within the grid's radius -- ``index`` (Qa,) int32, the lowest row on equal distance, -1 for none; ``dist``
    (Qa,) float32, +inf for none; ``count`` (Qa,) int32, the points within the radius.  ``skip_self``: the queries are the grid's own
    cloud (the same number of rows) and no row finds itself.  No synchronisation."""
    Q, scratch = _grid_handle(grid, "nearest_points")
    _on_device(queries, scratch, grid['points'])
    qs = _f32(queries, (None, 3), "queries")
    Qa = int(qs.shape[0])
    if Qa == 0:
        raise ValueError("nearest_points: no queries")
    if Qa > 2 ** 31 - 2:
        raise ValueError(f"nearest_points: {Qa} queries are beyond the kernel's limit of {2 ** 31 - 2}")
    if skip_self and Qa != Q:
        raise ValueError(f"nearest_points: skip_self with {Qa} queries against a grid of {Q} points (the queries must be the grid's cloud)")
    lib = _grid_scratch(grid, "nearest_points")
    dev = qs.device
    out = dict(index=torch.empty(Qa, dtype=torch.int32, device=dev), dist=torch.empty(Qa, dtype=torch.float32, device=dev),
               count=torch.empty(Qa, dtype=torch.int32, device=dev))
    _lib.check(lib.sp_cloud_grid_nearest(_lib.ptr(qs), Qa, Q, _lib.ptr(scratch), 1 if skip_self else 0, _lib.ptr(out['index']), _lib.ptr(out['dist']),
                                         _lib.ptr(out['count']), _lib.stream_ptr()), "sp_cloud_grid_nearest")
    return out


def _list_length(k, what):
    """``k`` as an int in 1 .. SP_CLOUD_KNN_MAX."""
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= _lib.SP_CLOUD_KNN_MAX:
        raise ValueError(f"{what}: k {k!r} (an integer in 1 .. {_lib.SP_CLOUD_KNN_MAX})")
    return k


def nearest_k(queries, grid, k, skip_self=False):
    """ONE ``sp_cloud_grid_knn`` call (include/sp_hip.h has the rule): per row of ``queries`` (Qa,3) float32 its ``k`` (1 .. 32) nearest
    points of the cloud behind ``grid`` (what ``cloud_grid`` returned) within the grid's radius -- ``index`` (Qa,k) int32, in ascending
    (distance, row) order, padded with -1; ``dist`` (Qa,k) float32, padded with +inf; ``count`` (Qa,) int32, ALL the points within the
    radius (what ``nearest_points`` counts).  ``skip_self``: the queries are the grid's own cloud (the same number of rows) and no row
    lists itself.  At ``k=1`` the result is ``nearest_points``' bit for bit.  No synchronisation."""
    Q, scratch = _grid_handle(grid, "nearest_k")
    k = _list_length(k, "nearest_k")
    _on_device(queries, scratch, grid['points'])
    qs = _f32(queries, (None, 3), "queries")
    Qa = int(qs.shape[0])
    if Qa == 0:
        raise ValueError("nearest_k: no queries")
    if Qa * k > 2 ** 31 - 2:
        raise ValueError(f"nearest_k: {Qa} lists of {k} are beyond the kernel's limit of {2 ** 31 - 2} entries")
    if skip_self and Qa != Q:
        raise ValueError(f"nearest_k: skip_self with {Qa} queries against a grid of {Q} points (the queries must be the grid's cloud)")
    lib = _grid_scratch(grid, "nearest_k")
    dev = qs.device
    out = dict(index=torch.empty(Qa, k, dtype=torch.int32, device=dev), dist=torch.empty(Qa, k, dtype=torch.float32, device=dev),
               count=torch.empty(Qa, dtype=torch.int32, device=dev))
    _lib.check(lib.sp_cloud_grid_knn(_lib.ptr(qs), Qa, Q, _lib.ptr(scratch), 1 if skip_self else 0, k, _lib.ptr(out['index']), _lib.ptr(out['dist']),
                                     _lib.ptr(out['count']), _lib.stream_ptr()), "sp_cloud_grid_knn")
    return out


def cloud_normals(points, radius, k=16, toward=None, owner=None, grid=None, origin=None):
    """A surface normal for every point of a cloud that has none: ``points`` (Q,3) float32 against itself -- ONE ``cloud_grid`` build at
    ``radius`` (unless ``grid``, a handle over these very points, is handed in; its radius then rules and ``radius`` / ``origin`` are
    ignored), ONE ``nearest_k`` with ``skip_self=False`` (the point itself is the first member of its list) and ONE ``sp_cloud_normals``
    launch (include/sp_hip.h has the rule): the eigenvector of the smallest eigenvalue of the covariance of the up to ``k`` (1 .. 32)
    nearest points within the radius, in float64.  ``toward``: (3,) or (V,3) float32 viewpoints; the normal of row i is turned towards
    ``toward[owner[i]]`` (``owner`` (Q,) int32; without it ``toward`` must be ONE viewpoint).  Without ``toward`` the component of
    largest magnitude is positive.  Returns ``dict(normals (Q,3) float32, curvature (Q,) float32, used (Q,) int32, knn)``: NaN normals
    and curvature where fewer than three points were in reach or they are coincident or collinear; ``knn`` is what ``nearest_k``
    returned.  No synchronisation."""
    k = _list_length(k, "cloud_normals")
    _on_device(points, toward, owner)
    pts = _f32(points, (None, 3), "points")
    Q = int(pts.shape[0])
    if Q == 0:
        raise ValueError("cloud_normals: no points")
    if grid is not None and (_grid_handle(grid, "cloud_normals")[0] != Q or grid['points'].device != pts.device):
        raise ValueError(f"cloud_normals: a grid of {int(grid['Q'])} points for a cloud of {Q}")
    view = own = None
    V = 0
    if toward is not None:
        if toward.dtype != torch.float32 or not (tuple(toward.shape) == (3,) or (toward.dim() == 2 and toward.shape[1] == 3 and toward.shape[0] >= 1)):
            raise ValueError(f"cloud_normals: toward must be float32 (3,) or (V,3), got {toward.dtype} {tuple(toward.shape)}")
        view = toward.detach().reshape(-1, 3).contiguous()
        V = int(view.shape[0])
        if owner is None and V != 1:
            raise ValueError(f"cloud_normals: {V} viewpoints need an owner per point")
        own = None if owner is None else _i32(owner, Q, "owner")
    elif owner is not None:
        raise ValueError("cloud_normals: owner without toward")
    if grid is None:
        grid = cloud_grid(pts, radius, origin)
    knn = nearest_k(grid['points'], grid, k)
    lib = _lib.load()
    dev = pts.device
    out = dict(normals=torch.empty(Q, 3, dtype=torch.float32, device=dev), curvature=torch.empty(Q, dtype=torch.float32, device=dev),
               used=torch.empty(Q, dtype=torch.int32, device=dev), knn=knn)
    _lib.check(lib.sp_cloud_normals(_lib.ptr(grid['points']), Q, _lib.ptr(grid['points']), _lib.ptr(knn['index']), Q, k, _lib.ptr(view), V, _lib.ptr(own),
                                    _lib.ptr(out['normals']), _lib.ptr(out['curvature']), _lib.ptr(out['used']), _lib.stream_ptr()), "sp_cloud_normals")
    return out


_RESIDUALS = {'point': 0, 'plane': 1, 'query_plane': 2}


def register_clouds(queries, grid, normals=None, residual='point', T0=None, s0=1.0, scale=False, huber=None, tol=1e-6, min_pairs=None, max_iters=30):
    """ONE ``sp_cloud_register`` call (include/sp_hip.h has the rule): the similarity x -> s R x + t that moves ``queries`` (Qa,3)
    float32 onto the cloud behind ``grid`` (what ``cloud_grid`` returned; its radius is the correspondence radius), by Gauss-Newton ICP
    from the start ``T0`` ((4,4), rotation and translation; default the identity) and ``s0``.  ``residual``: ``'point'`` (point to
    point), ``'plane'`` (point to plane: ``normals`` (Q,3) float32, one row per GRID point) or ``'query_plane'`` (``normals`` (Qa,3)
    float32, one row per QUERY: a map with normals against a cloud without).  ``scale``: the scale is an unknown too; ``huber``: the
    Huber threshold (None or 0: every pair weighs 1); ``tol``: the step length at which it stops; ``min_pairs``: fewer pairs end it
    (default: the number of unknowns); ``max_iters`` iterations are enqueued and the stop is decided on the device.
    Returns ``dict(rot (3,3), trans (3,), s (), T (4,4) = [[s R, t], [0, 1]]`` float64, ``status`` () int32 (``_lib.SP_CLOUD_REG_*``),
    ``iterations`` () int32, ``n`` () int64 (pairs of the last iteration), ``cost`` () float64, ``history`` (max_iters,4) float64 rows
    {n, cost, step, status}, ``index`` (Qa,) int32 the last correspondences (-1: none))``, all on the device (views of one record).  No synchronisation, no host read."""
    Q, scratch = _grid_handle(grid, "register_clouds")
    if residual not in _RESIDUALS:
        raise ValueError(f"register_clouds: residual {residual!r} (one of {sorted(_RESIDUALS)})")
    kind = _RESIDUALS[residual]
    if kind != 0 and normals is None:
        raise ValueError(f"register_clouds: residual {residual!r} needs normals")
    _on_device(queries, scratch, grid['points'], normals if kind != 0 else None)
    qs = _f32(queries, (None, 3), "queries")
    Qa = int(qs.shape[0])
    if Qa == 0:
        raise ValueError("register_clouds: no queries")
    if Qa > 2 ** 31 - 2:
        raise ValueError(f"register_clouds: {Qa} queries are beyond the kernel's limit of {2 ** 31 - 2}")
    nrm = None
    if kind != 0:
        rows = Q if kind == 1 else Qa
        nrm = _f32(normals, (rows, 3), f"normals (one row per {'grid point' if kind == 1 else 'query'})")
    unknowns = 7 if scale else 6
    try:
        huber = 0.0 if huber is None else float(huber)
        tol, s0 = float(tol), float(s0)
        min_pairs = unknowns if min_pairs is None else int(min_pairs)
        max_iters = int(max_iters)
    except (TypeError, ValueError) as e:
        raise ValueError(f"register_clouds: huber {huber!r}, tol {tol!r}, s0 {s0!r}, min_pairs {min_pairs!r}, max_iters {max_iters!r}: {e}") from None
    if not (0.0 <= huber < float("inf")) or not (0.0 <= tol < float("inf")) or not (0.0 < s0 < float("inf")):
        raise ValueError(f"register_clouds: huber {huber}, tol {tol} (finite, >= 0), s0 {s0} (finite, > 0)")
    if min_pairs < unknowns or not 1 <= max_iters <= _lib.SP_CLOUD_REG_ITERS_LIMIT:
        raise ValueError(f"register_clouds: min_pairs {min_pairs} (>= {unknowns} unknowns), max_iters {max_iters} (1 .. {_lib.SP_CLOUD_REG_ITERS_LIMIT})")
    dev = qs.device
    try:
        start = torch.eye(4, dtype=torch.float64) if T0 is None else torch.as_tensor(T0, dtype=torch.float64).detach()
    except (TypeError, ValueError) as e:
        raise ValueError(f"register_clouds: T0 {T0!r}: {e}") from None
    if tuple(start.shape) != (4, 4):
        raise ValueError(f"register_clouds: T0 must be (4,4), got {tuple(start.shape)}")
    lib = _grid_scratch(grid, "register_clouds")
    start = start.to(dev)
    state = torch.zeros(64, dtype=torch.float64, device=dev)
    state[:9] = start[:3, :3].reshape(9)
    state[9:12] = start[:3, 3]
    state[12] = s0
    history = torch.empty(max_iters, 4, dtype=torch.float64, device=dev)
    index = torch.empty(Qa, dtype=torch.int32, device=dev)
    work = torch.empty(lib.sp_cloud_register_work_doubles(Qa), dtype=torch.float64, device=dev)
    _lib.check(lib.sp_cloud_register(_lib.ptr(qs), _lib.ptr(nrm), Qa, Q, _lib.ptr(scratch), kind, 1 if scale else 0, huber, tol, min_pairs, max_iters,
                                     _lib.ptr(state), _lib.ptr(history), _lib.ptr(index), _lib.ptr(work), _lib.stream_ptr()), "sp_cloud_register")
    rot, trans, s = state[:9].view(3, 3), state[9:12], state[12]
    T = torch.zeros(4, 4, dtype=torch.float64, device=dev)
    T[:3, :3] = s * rot
    T[:3, 3] = trans
    T[3, 3] = 1.0
    words = state.view(torch.int32)
    return dict(rot=rot, trans=trans, s=s, T=T, status=words[2 * 58], iterations=words[2 * 58 + 1], n=state.view(torch.int64)[57], cost=state[55],
                history=history, index=index)


def _volume(volume, what):
    """What ``odometery.results.tsdf_volume`` returned, checked: (tsdf, weight, colour or None, (nx, ny, nz), voxel, origin, trunc) with the
    three numbers as the float32 the kernel reads.  The state tensors are updated in place, so they must be contiguous as they are."""
    if not isinstance(volume, dict) or any(k not in volume for k in ('tsdf', 'weight', 'colour', 'origin', 'voxel', 'trunc', 'dims')):
        raise ValueError(f"{what}: volume must be what tsdf_volume returned")
    tsdf, weight, colour = volume['tsdf'], volume['weight'], volume['colour']
    try:
        nx, ny, nz = (int(n) for n in volume['dims'])
        vox, trunc = (float(torch.tensor(float(volume[k]), dtype=torch.float32)) for k in ('voxel', 'trunc'))
        org = [float(o) for o in torch.as_tensor(volume['origin'], dtype=torch.float64).reshape(-1).float().tolist()]
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"{what}: volume dims {volume['dims']!r}, voxel {volume['voxel']!r}, trunc {volume['trunc']!r}, origin {volume['origin']!r}: {e}") from None
    if min(nx, ny, nz) < 1 or nx * ny * nz > _lib.SP_TSDF_MAX_NODES:
        raise ValueError(f"{what}: a volume of {nx}x{ny}x{nz} nodes (1 .. 2^30 in all)")
    if not (0.0 < vox < float("inf")) or not (0.0 < trunc < float("inf")):
        raise ValueError(f"{what}: voxel {volume['voxel']}, trunc {volume['trunc']} (finite float32 > 0)")
    if len(org) != 3 or not all(abs(o) < float("inf") for o in org):
        raise ValueError(f"{what}: origin {volume['origin']} (three finite float32 numbers)")
    for name, t, shape in (('tsdf', tsdf, (nz, ny, nx)), ('weight', weight, (nz, ny, nx)), ('colour', colour, (nz, ny, nx, 3))):
        if t is None and name == 'colour':
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{what}: volume['{name}'] must be a contiguous float32 tensor {shape}")
    return tsdf, weight, colour, (nx, ny, nz), vox, org, trunc


def _min_weight(what, min_weight, nx, ny, nz):
    """``min_weight``, a float already, is not NaN, and the volume has a cell."""
    if min_weight != min_weight:
        raise ValueError(f"{what}: min_weight is NaN")
    if min(nx, ny, nz) < 2:
        raise ValueError(f"{what}: a volume of {nx}x{ny}x{nz} nodes has no cell (every size must be >= 2)")


def tsdf_integrate(volume, depths, Ks, poses, images=None, z_min=Z_MIN, depth_max=float("inf")):
    """ONE ``sp_tsdf_integrate`` launch (include/sp_hip.h has the rule): ``depths`` (V,H,W) float32 fused into ``volume`` (what
    ``odometery.results.tsdf_volume`` returned) IN PLACE, view after view; ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4) camera-to-world in the
    volume's frame, ``images`` (V,3,H,W) float32 or None -- without them the volume's colour, if it has one, is left untouched.  A depth
    counts iff it is finite and 0 < d <= ``depth_max``; a node is tested against a view iff its z there is > ``z_min``.  Returns
    ``volume``.  No synchronisation."""
    tsdf, weight, colour, (nx, ny, nz), vox, org, trunc = _volume(volume, "tsdf_integrate")
    _on_device(tsdf, weight, colour, depths, Ks, poses, images)
    V = _view_count(poses, "tsdf_integrate")
    d = _f32(depths, (V, None, None), "depths")
    views, H, W = _view_set(Ks, poses, V, d.shape[1], d.shape[2])
    img = None
    if images is not None:
        if colour is None:
            raise ValueError("tsdf_integrate: images for a volume without colour")
        img = _f32(images, (V, 3, H, W), "images")
    _z_min(z_min)
    if not float(depth_max) > 0.0:
        raise ValueError(f"tsdf_integrate: depth_max {depth_max} (> 0; inf allowed)")
    _limits("tsdf_integrate", V, H, W)
    lib = _lib.load()
    _lib.check(lib.sp_tsdf_integrate(_lib.ptr(d), _lib.ptr(img), _lib.ptr(views), V, H, W, nx, ny, nz, vox, org[0], org[1], org[2], trunc,
                                     float(z_min), float(depth_max), _lib.ptr(tsdf), _lib.ptr(weight), _lib.ptr(colour if img is not None else None),
                                     _lib.stream_ptr()), "sp_tsdf_integrate")
    return volume


def tsdf_mesh(volume, min_weight=1.0):
    """The zero level set of ``volume`` as an indexed triangle mesh (``sp_tsdf_mesh``; include/sp_hip.h has the rule): a counting call,
    ONE host read of the two counts (the one synchronisation), buffers of exactly that size, and a second call that fills them.  A node
    counts iff its weight is >= ``min_weight`` and its tsdf is finite.  Returns ``dict(vertices (n,3) float32, colours (n,3) float32 or
    None -- for a volume without colour --, faces (F,3) int32)``; faces look into free space."""
    tsdf, weight, colour, (nx, ny, nz), vox, org, _ = _volume(volume, "tsdf_mesh")
    _on_device(tsdf, weight, colour)
    try:
        min_weight = float(min_weight)
    except (TypeError, ValueError) as e:
        raise ValueError(f"tsdf_mesh: min_weight {min_weight!r}: {e}") from None
    _min_weight("tsdf_mesh", min_weight, nx, ny, nz)
    lib = _lib.load()
    dev = tsdf.device
    scratch = torch.empty(lib.sp_tsdf_mesh_scratch_bytes(nx, ny, nz) // 4, dtype=torch.int32, device=dev)
    n_out = torch.empty(2, dtype=torch.int64, device=dev)

    def call(nv, nf, vertices, colours, faces):
        _lib.check(lib.sp_tsdf_mesh(_lib.ptr(tsdf), _lib.ptr(weight), _lib.ptr(colour), nx, ny, nz, vox, org[0], org[1], org[2], min_weight,
                                    _lib.ptr(scratch), nv, nf, _lib.ptr(vertices), _lib.ptr(colours), _lib.ptr(faces), _lib.ptr(n_out),
                                    _lib.stream_ptr()), "sp_tsdf_mesh")
    call(0, 0, None, None, None)
    nv, nf = (int(n) for n in n_out.tolist())                                    # the one host read
    if nv > 2 ** 31 - 1 or nf > 2 ** 31 - 1:
        raise ValueError(f"tsdf_mesh: {nv} vertices and {nf} faces are beyond 32-bit indices")
    out = dict(vertices=torch.empty(nv, 3, dtype=torch.float32, device=dev),
               colours=None if colour is None else torch.empty(nv, 3, dtype=torch.float32, device=dev),
               faces=torch.empty(nf, 3, dtype=torch.int32, device=dev))
    if nv > 0:
        call(nv, nf, out['vertices'], out['colours'], out['faces'] if nf > 0 else None)
    return out


def tsdf_raycast(volume, Ks, poses, H, W, z_max, min_weight=1.0, z_min=Z_MIN, step=None, depth=True, normals=True, image=None, index=True):
    """ONE ``sp_tsdf_raycast`` launch (include/sp_hip.h has the rule): ``volume`` (what ``odometery.results.tsdf_volume`` returned, fused)
    seen from V cameras, ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4) camera-to-world in the volume's frame.  One ray per pixel, sampled at
    the camera depths ``z_min + k step``, ``k = 0 .. n_steps-1`` with ``n_steps = ceil((z_max - z_min) / step) + 1`` (``step`` defaults to
    the volume's voxel); the first valid sample with a negative field ends it, and it is a hit iff the sample before is valid and not
    negative.  A node counts iff its weight is >= ``min_weight`` and its tsdf is finite.  Returns the requested of ``depth`` (V,H,W)
    float32 (0 without a hit), ``normals`` (V,H,W,3) float32 in the volume's frame, facing the cameras that saw the surface (NaN without
    a hit, or where a neighbouring cell is unobserved), ``image`` (V,H,W,3) uint8 (0) and ``index`` (V,H,W) int32, the lower node of the
    cell behind the surface (-1), as a dict.  ``image=None``: an image iff the volume has a colour; ``image=True`` for a volume without
    one is an error.  No synchronisation."""
    tsdf, weight, colour, (nx, ny, nz), vox, org, _ = _volume(volume, "tsdf_raycast")
    _on_device(tsdf, weight, colour, Ks, poses)
    V = _view_count(poses, "tsdf_raycast")
    views, H, W = _view_set(Ks, poses, V, H, W)
    try:
        min_weight, z_min, z_max = float(min_weight), float(z_min), float(z_max)
        step = vox if step is None else float(torch.tensor(float(step), dtype=torch.float32))
    except (TypeError, ValueError) as e:
        raise ValueError(f"tsdf_raycast: min_weight {min_weight!r}, z_min {z_min!r}, z_max {z_max!r}, step {step!r}: {e}") from None
    _z_min(z_min)
    _min_weight("tsdf_raycast", min_weight, nx, ny, nz)
    if not (0.0 < step < float("inf")):
        raise ValueError(f"tsdf_raycast: step {step} (finite float32 > 0)")
    if not (z_min < z_max < float("inf")):
        raise ValueError(f"tsdf_raycast: depth range z_min {z_min} .. z_max {z_max} (z_min < z_max, both finite)")
    steps = (z_max - z_min) / step
    if not steps < _lib.SP_TSDF_RAYCAST_MAX_STEPS:
        raise ValueError(f"tsdf_raycast: {steps:.3g} steps of {step} from {z_min} to {z_max} are beyond the kernel's limit of 2^20")
    n_steps = int(-(-steps // 1)) + 1
    if image and colour is None:
        raise ValueError("tsdf_raycast: an image needs a volume with colour")
    image = colour is not None if image is None else bool(image)
    if not (depth or normals or image or index):
        raise ValueError("tsdf_raycast: no output asked for")
    _limits("tsdf_raycast", V, H, W)
    lib = _lib.load()
    out = _view_images(V, H, W, tsdf.device, depth=depth, normals=normals, image=image, index=index)
    _lib.check(lib.sp_tsdf_raycast(_lib.ptr(tsdf), _lib.ptr(weight), _lib.ptr(colour), nx, ny, nz, vox, org[0], org[1], org[2], min_weight,
                                   _lib.ptr(views), V, H, W, z_min, step, n_steps, _lib.ptr(out.get('depth')), _lib.ptr(out.get('normals')),
                                   _lib.ptr(out.get('image')), _lib.ptr(out.get('index')), _lib.stream_ptr()), "sp_tsdf_raycast")
    return out


def _mesh(vertices, faces, what):
    """(vertices (M,3) float32, faces (F,3) int32) contiguous, on one device, within the kernels' limits."""
    _on_device(vertices, faces)
    v = _f32(vertices, (None, 3), f"{what}: vertices")
    if faces.dtype != torch.int32 or faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError(f"{what}: faces must be int32 (F,3), got {faces.dtype} {tuple(faces.shape)}")
    M, F = int(v.shape[0]), int(faces.shape[0])
    if M < 1 or F < 1:
        raise ValueError(f"{what}: a mesh of {M} vertices and {F} faces")
    if M > _lib.SP_MESH_MAX_FACES or F > _lib.SP_MESH_MAX_FACES:
        raise ValueError(f"{what}: {M} vertices and {F} faces are beyond the kernel's limit of 2^28")
    return v, faces.detach().contiguous(), M, F


def mesh_faces(vertices, faces, cross=False):
    """ONE ``sp_mesh_faces`` launch (include/sp_hip.h has the rule): per face of ``vertices`` (M,3) float32, ``faces`` (F,3) int32 its
    ``state`` (F,) uint8 (0 valid, 1 an index outside the vertices, 2 a repeated index, 3 a non-finite coordinate, 4 zero area), ``area``
    (F,) float64 and unit ``normals`` (F,3) float32 -- zeros unless the state is 0 --, with ``cross`` also the raw cross product (F,3)
    float64; and ``summary`` (6,) int64: the faces of each state and the bits of the largest area (``summary[5:].view(torch.float64)``).
    No synchronisation."""
    v, f, M, F = _mesh(vertices, faces, "mesh_faces")
    dev = v.device
    out = dict(area=torch.empty(F, dtype=torch.float64, device=dev), normals=torch.empty(F, 3, dtype=torch.float32, device=dev),
               state=torch.empty(F, dtype=torch.uint8, device=dev), summary=torch.empty(_lib.SP_MESH_SUMMARY_WORDS, dtype=torch.int64, device=dev))
    if cross:
        out['cross'] = torch.empty(F, 3, dtype=torch.float64, device=dev)
    lib = _lib.load()
    _lib.check(lib.sp_mesh_faces(_lib.ptr(v), M, _lib.ptr(f), F, _lib.ptr(out['area']), _lib.ptr(out['normals']), _lib.ptr(out['state']),
                                 _lib.ptr(out.get('cross')), _lib.ptr(out['summary']), _lib.stream_ptr()), "sp_mesh_faces")
    return out


def _density_seed(density, seed, what):
    try:
        whole = int(seed)
        if whole != seed:
            raise ValueError("the seed must be a whole number")
        density, seed = float(density), whole
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: density {density!r}, seed {seed!r}: {e}") from None
    if not (0.0 < density < float("inf")):
        raise ValueError(f"{what}: density {density} (finite, > 0)")
    if not -2 ** 63 <= seed < 2 ** 64:
        raise ValueError(f"{what}: seed {seed} is not 64 bits")
    seed &= 2 ** 64 - 1
    return density, seed - 2 ** 64 if seed >= 2 ** 63 else seed                    # (the same 64 bits as the signed integer the ABI carries)


def mesh_sample(vertices, faces, records, density, seed=0, colours=None):
    """An area-uniform, seeded cloud of the mesh (``sp_mesh_sample``; include/sp_hip.h has the rule): ``records`` is what ``mesh_faces``
    returned for this mesh, ``density`` the samples per unit area, ``colours`` (M,3) float32 vertex colours or None.  A counting call, ONE
    host read of the count (the one synchronisation), buffers of exactly that size, and a second call that fills them.  Returns
    ``dict(points, normals (N,3) float32, colours (N,3) float32 or None, face (N,) int32)``, rows ordered by (face, sample); the same
    arguments give the same bits."""
    v, f, M, F = _mesh(vertices, faces, "mesh_sample")
    density, seed = _density_seed(density, seed, "mesh_sample")
    if not isinstance(records, dict) or any(not torch.is_tensor(records.get(k)) for k in ('area', 'normals', 'state')):
        raise ValueError("mesh_sample: records must be what mesh_faces returned")
    area, nrm, state = records['area'], records['normals'], records['state']
    if area.dtype != torch.float64 or tuple(area.shape) != (F,) or state.dtype != torch.uint8 or tuple(state.shape) != (F,) \
            or nrm.dtype != torch.float32 or tuple(nrm.shape) != (F, 3):
        raise ValueError(f"mesh_sample: records of another mesh: area {tuple(area.shape)}, normals {tuple(nrm.shape)}, state {tuple(state.shape)} for {F} faces")
    cols = None if colours is None else _f32(colours, (M, 3), "mesh_sample: colours")
    _on_device(v, f, area, nrm, state, cols)
    area, nrm, state = area.contiguous(), nrm.contiguous(), state.contiguous()
    lib = _lib.load()
    dev = v.device
    scratch = torch.empty(8 * lib.sp_mesh_sample_scratch_units(F), dtype=torch.int64, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)

    def call(cap, points, normals, out_colours, face):
        _lib.check(lib.sp_mesh_sample(_lib.ptr(v), _lib.ptr(cols), M, _lib.ptr(f), F, _lib.ptr(area), _lib.ptr(nrm), _lib.ptr(state), density, seed,
                                      _lib.ptr(scratch), cap, _lib.ptr(points), _lib.ptr(normals), _lib.ptr(out_colours), _lib.ptr(face),
                                      _lib.ptr(n_out), _lib.stream_ptr()), "sp_mesh_sample")
    call(0, None, None, None, None)
    N = int(n_out.item())                                                        # the one host read
    if N > 2 ** 31 - 1:
        raise ValueError(f"mesh_sample: {N} samples are beyond 32-bit rows; lower the density")
    out = dict(points=torch.empty(N, 3, dtype=torch.float32, device=dev), normals=torch.empty(N, 3, dtype=torch.float32, device=dev),
               colours=None if cols is None else torch.empty(N, 3, dtype=torch.float32, device=dev),
               face=torch.empty(N, dtype=torch.int32, device=dev))
    if N > 0:
        call(N, out['points'], out['normals'], out['colours'], out['face'])
    return out


def mesh_render(vertices, faces, Ks, poses, H, W, colours=None, face_normals=None, z_min=Z_MIN, cull=False, depth=True, normals=None, image=None,
                index=True):
    """ONE ``sp_mesh_render`` call (include/sp_hip.h has the rule): the mesh ``vertices`` (M,3) float32, ``faces`` (F,3) int32 rasterised
    into V views, ``Ks`` (V,3,3) or (3,3), ``poses`` (V,4,4) camera-to-world in the mesh's frame.  A pixel whose centre lies inside a face
    (edges included: no cracks between neighbours) at a camera depth > ``z_min`` is contested through the depth buffer: the nearest face
    wins, equal depths go to the highest face.  ``cull=True`` keeps only faces seen from their front, the side their ``mesh_faces`` normal
    points to.  ``colours`` (M,3) float32 vertex colours in 0..1, ``face_normals`` (F,3) float32 (``mesh_faces``' ``normals``).  Returns
    the requested of ``depth`` (V,H,W) float32 (0 where no face lies), ``normals`` (V,H,W,3) float32, the winning face's (NaN there),
    ``image`` (V,H,W,3) uint8, interpolated perspective-correctly (0) and ``index`` (V,H,W) int32, the winning face (-1), as a dict.
    ``normals=None`` / ``image=None``: that output iff ``face_normals`` / ``colours`` is given; asking for one without its input is an
    error.  No synchronisation."""
    v, f, M, F = _mesh(vertices, faces, "mesh_render")
    _on_device(v, f, Ks, poses, colours, face_normals)
    V = _view_count(poses, "mesh_render")
    views, H, W = _view_set(Ks, poses, V, H, W)
    try:
        z_min = float(z_min)
    except (TypeError, ValueError) as e:
        raise ValueError(f"mesh_render: z_min {z_min!r}: {e}") from None
    _z_min(z_min)
    cols = None if colours is None else _f32(colours, (M, 3), "mesh_render: colours")
    nrm = None if face_normals is None else _f32(face_normals, (F, 3), "mesh_render: face_normals")
    if image and cols is None:
        raise ValueError("mesh_render: an image needs colours")
    if normals and nrm is None:
        raise ValueError("mesh_render: normals need face_normals (mesh_faces' normals)")
    image = cols is not None if image is None else bool(image)
    normals = nrm is not None if normals is None else bool(normals)
    if not (depth or normals or image or index):
        raise ValueError("mesh_render: no output asked for")
    _limits("mesh_render", V, H, W)
    lib = _lib.load()
    dev = v.device
    scratch = torch.empty(8 * lib.sp_mesh_render_scratch_units(F), dtype=torch.int64, device=dev)
    keys = torch.empty(V * H * W, dtype=torch.int64, device=dev)
    out = _view_images(V, H, W, dev, depth=depth, normals=normals, image=image, index=index)
    _lib.check(lib.sp_mesh_render(_lib.ptr(v), _lib.ptr(cols), M, _lib.ptr(f), F, _lib.ptr(nrm), _lib.ptr(views), V, H, W, z_min, 1 if cull else 0,
                                  _lib.ptr(scratch), _lib.ptr(keys), _lib.ptr(out.get('depth')), _lib.ptr(out.get('normals')),
                                  _lib.ptr(out.get('image')), _lib.ptr(out.get('index')), _lib.stream_ptr()), "sp_mesh_render")
    return out
